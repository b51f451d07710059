"""GPU: the kernels that turn numbers into a CHOICE, each alone through its C entry, against plain models
(tests/choice_models.py, tests/test_speaker_beam_device_host.py) on constructed inputs: exact ties, lists shorter than
the beam, rows with one valid candidate, ragged widths, logits far from zero.

    1  sf_speaker_beam_select      bit for bit against `model_step`, every buffer after every launch, poison in the
                                   places the contract does not name
    2  sf_speaker_glue_fwd / sf_follower_glue_fwd, feedback 0 and 1
                                   choices and flags exact; score / NLL / CE by the rule below
    3  sf_speaker_glue_bwd / sf_follower_glue_bwd
                                   gscale * (softmax - onehot) against float64, padding columns written zero
    4  sf_reduce_terms + sf_loss_finalize
                                   against float64 sums with a priori bounds (choice_models.reduce_bound /
                                   finalize_bound), steps without a live row, the entries behind T untouched
    (5, sf_logprob_topk at its edges, stands beside the older tests of that entry in tests/test_gpu_search.py)
    6  sf_follower_glue_fwd, feedback 2 (the sampled action), and u_next at every feedback
                                   draw by draw against the float64 mirror oracle.rng.follower_sample at the row's own
                                   uniform; chi-square against softmax; addressing by global row, stream and site
                                   word; u_next = the chosen row times the next step's dropout mask, bit for bit

The draw-by-draw rule of section 6 (choice_models.check_draws): a row whose margin -- the smallest distance of u to a
boundary of the float64 cdf -- exceeds 1e-5 is CLEAR and must take the mirror's action; an unclear row must take one of
the mirror's actions at u * (1 - 1e-5) and u * (1 + 1e-5); no row is skipped; every action is a valid candidate with a
finite logit and a float32 weight above 0.  The cases keep a clear share of at least 0.99 (asserted on the mirror alone
in tests/test_choice_models_host.py).

A bug this section found, fixed with it (csrc/sf_glue.h, follower_glue_row): the draw took the first valid lane whose
float32 prefix sum exceeded u * sum, or the highest valid lane when none did.  Every lane's prefix sum is rounded in an
order of its own, so behind the last candidate that carries weight the sums of an underflowed tail (expf gives 0 below
-104) are level only up to an ulp: at u = 1 - 2^-24 the device drew a tail candidate -- probability exactly 0 in float32,
below 1e-45 in float64 -- in 3 of the 6 rows built for it (A 9: candidate 7 of a tail 5..8; A 16: 15; A 64: 32, the first
behind the head), through the hit as well as through the fallback.  Now only a lane with e > 0 can be drawn.

Float outputs that are differences of logits and a log-sum-exp follow the rule of tests/grad_compare.py: with r the
float64 model and f the same formula in numpy float32, e = max|got - r| <= max(K * max|f - r|, 1e-5), K = 4.  Every
case prints e and e32 (pytest -s).  Nothing is skipped or filtered: rows without a tie are built with a gap of at
least 1e-3 between the best and the second value.

Measured on an MI355X (e / e32, the worst case of each group; nothing came near its bound):

    glue forward, rows not shifted      1.12e-06 / 1.12e-06   speaker, vocab 991, teacher, score        (bound 1.0e-05)
    glue forward, rows shifted +-80     3.96e-06 / 3.92e-06   follower, A 64, teacher, -80, score       (bound 1.6e-05)
    glue forward, rows shifted +1e4     4.88e-04 / 4.88e-04   follower, A 9, teacher, score             (bound 2.0e-03)
    glue backward (relative)            8.85e-08 / 7.08e-08   speaker, vocab 1024, gscale 1/7, -80      (bound 2.0e-06)
    top-k log-probabilities             2.03e-06 / 1.46e-06   n 991, k 991, not shifted                 (bound 1.0e-05)
                                        7.79e-07 / 4.81e-04   n 991, k 991, +1e4: the kernel subtracts the row maximum
                                                              before the log-sum, the float32 model adds it back first
    loss                                4.92e-05 at T 130, B 1000 (a priori bound 2.5e-03); counts, gscale zeros exact
    sampled score, rows not shifted     6.29e-07 / 5.05e-07   A 64, a_num, the u = 0 launch                (bound 1.0e-05)
    sampled score, rows shifted +-80    4.00e-06 / 3.87e-06   A 64, is_valid, +80                         (bound 1.5e-05)
    sampled score, rows shifted +1e4    4.88e-04 / 4.88e-04   A 64, is_valid, the u = 0.5 launch          (bound 2.0e-03)
    clear share of the draws            1.0000 in the 12 ordinary launches and the 8 with the u = 0 row (3 320 rows: no
                                        unclear row came up); 127 / 128 and 255 / 256 where the u = 1 - 2^-24 or the
                                        u = 0.5 row is unclear by construction; 0.9986 .. 0.9999 over the 40 000 rows
                                        of a chi-square case (p-values 0.039 .. 0.54).  Every clear row took the
                                        mirror's action.

The shifted rows cost what float32 costs there -- one step of a logit near 1e4 is 9.8e-04 -- and the kernels stay within
the float32 model's own error.  The whole module (216 tests) takes about 6 s of wall time, 0.7 s of it in its slowest
test (the first chi-square case: 40 000 rows and scipy's import).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_speaker_beam_device_host as M           # noqa: E402  (the beam selection's numpy model and its scenarios)
from tests import choice_models as CM               # noqa: E402
from tests import grad_compare                       # noqa: E402

F32 = np.float32
POISON = M.POISON


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def poison_f32(*shape):
    return np.full(shape, POISON, np.int32).view(F32)


# ------------------------------------------------------------------------------------------ 1. the beam selection
@pytest.mark.parametrize('B,beam', [(1, 1), (1, 3), (64, 3), (1, 40), (64, 40), (1, 64), (64, 64)])
def test_speaker_beam_select_equals_its_numpy_model_bit_for_bit(B, beam):
    """sf_speaker_beam_select alone over T + 2 launches per scenario (test_speaker_beam_device_host.SCENARIOS): exact
    score ties across slots and inside one list, EOS at t = 0, finals by the last step, a completion list that fills
    while hypotheses still continue, live * k < beam_size with k < beam_size, -inf log-probabilities, instances that
    end at different steps, launches after the end, the attention history present and absent, ld_hist at and above
    its minimum.  Exact: the only arithmetic is one float32 add.  hist_attn is compared whole, so alpha[i] landing at
    the GLOBAL slot i (base + the slot's place in its instance) is pinned."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    Tp = 4
    trace = {}
    names = ('score', 'words', 'parent', 'inst', 'live_total', 'hist_word', 'hist_parent', 'hist_score', 'hist_attn',
             'done_rec', 'done_score')
    for name in M.SCENARIOS:
        rng = np.random.default_rng([B, beam, M.SCENARIOS.index(name)])
        k, T, with_attn, ld = M.scenario_shape(name, B, beam, Tp)
        s = M.new_state(B, beam, T, Tp, with_attn=with_attn, ld=ld)
        d = {n: up(s[n]) for n in names if s[n] is not None}
        sb = _lib.SpkBeam(B, beam, k, T, Tp, s['eos'], *(d[n].data_ptr() if n in d else None for n in names[:9]), ld,
                          d['done_rec'].data_ptr(), d['done_score'].data_ptr())
        for step in range(T + 2):
            top_w, top_lp, alpha = M.scenario_inputs(rng, s, k, name, step)
            M.model_step(s, top_w, top_lp, alpha if with_attn else None, trace)
            d_w, d_lp, d_alpha = up(top_w), up(top_lp), up(alpha)
            call('sf_speaker_beam_select', C.byref(sb), ptr(d_w), ptr(d_lp), ptr(d_alpha) if with_attn else None, stream())
            for n in d:
                got = down(d[n])
                assert got.shape == s[n].shape and got.dtype == s[n].dtype, (name, step, n)
                assert np.array_equal(bits(got), bits(s[n])), (name, step, n)
        assert (s['inst'][:, 0] == 0).all() and (s['inst'][:, 2] <= T).all()
        assert (bits(s['hist_word']) == POISON).any()             # (places no launch named are there to be watched)
    M.scenario_expectations(trace, B, beam)


# ------------------------------------------------------------------------------------- 2. the per-step glue, forward
def run_speaker_glue(case, feedback, ldv):
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    x = case['logit']
    B, vocab = x.shape
    lg = np.empty((B, ldv), F32)
    lg[:, :vocab] = x
    lg[:, vocab:] = np.where(np.arange(ldv - vocab) % 2 == 0, np.nan, 1e30).astype(F32)    # read them and fail
    d_lg, d_t, d_e = up(lg), up(case['target']), up(case['ended'])
    d_w = up(np.full(B, -7, np.int64))
    d_s, d_n, d_l = up(poison_f32(B)), up(poison_f32(B)), up(poison_f32(B))
    call('sf_speaker_glue_fwd', B, vocab, ldv, ptr(d_lg), ptr(d_t), feedback, case['pad'], case['eos'], ptr(d_e),
         ptr(d_w), ptr(d_s), ptr(d_n), ptr(d_l), None, stream())
    assert np.array_equal(bits(down(d_lg)), bits(lg))               # the logits are read only
    return dict(w=down(d_w), ended=down(d_e), score=down(d_s), nll=down(d_n), live=down(d_l))


@pytest.mark.parametrize('feedback', [0, 1])
@pytest.mark.parametrize('vocab', [1, 2, 63, 64, 65, 991, 1024, 1025, 1500])
def test_speaker_glue_fwd_against_the_reference_lines(vocab, feedback):
    """speaker.py:163-191 per row: the word (teacher: the target; argmax: the lowest index among the maxima of the
    float32 row, with the maximum duplicated across lanes, inside one lane's columns and across column 1023 / 1024),
    score, NLL term, liveness, and `ended` set for exactly the rows whose word is EOS."""
    for seed in range(2 if vocab == 1 else 1):
        case = CM.speaker_glue_case(vocab, seed)
        ldv = ((vocab + 3) & ~3) + 4
        got = run_speaker_glue(case, feedback, ldv)
        args = (case['logit'], case['target'], feedback, case['pad'], case['eos'], case['ended'])
        r, f = CM.speaker_glue(*args, np.float64), CM.speaker_glue(*args, F32)
        if feedback == 1:
            assert np.array_equal(r['w'], case['best'])               # (the construction and the model agree)
            assert case['tie'].any() or vocab == 1
        assert np.array_equal(got['w'], r['w'])
        assert np.array_equal(got['ended'], r['ended'])
        hit = r['w'] == case['eos']
        assert vocab == 1 or (hit.any() and (case['ended'][~hit] == 0xA5).any() and (case['ended'][hit] != 1).any())
        assert np.array_equal(bits(got['live']), bits(r['live']))
        assert vocab == 1 or ((r['live'] == 0).any() and (r['live'] == 1).any())
        what = 'speaker glue fwd vocab %d feedback %d' % (vocab, feedback)
        for sh in CM.SHIFTS:
            rows = case['shift'] == sh
            for key in ('score', 'nll'):
                CM.check_values('%s shift %g %s' % (what, sh, key), got[key][rows], r[key][rows], f[key][rows])
        pad_word = r['w'] == case['pad']
        assert not got['score'][pad_word].any() and not got['nll'][r['live'] == 0].any()       # exact zeros


def run_follower_glue(case, feedback, via_a_num):
    from speaker_follower_amd import _lib
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    x = case['logit']
    B, A = x.shape
    d_lg, d_t, d_e = up(x), up(case['target']), up(case['ended'])
    d_valid = up(case['valid'].astype(F32))
    d_anum = up(case['a_num'])
    d_a, d_tu = up(np.full(B, -7, np.int64)), up(np.full(B, -7, np.int64))
    d_s, d_ce, d_l = up(poison_f32(B)), up(poison_f32(B)), up(poison_f32(B))
    d_u = torch.zeros(B, A, 4, device='cuda')                         # (never read: u_next is NULL)
    cands = _lib.Cands(d_u.data_ptr(), None, None, None, None, d_anum.data_ptr() if via_a_num else None, A, 1, 4, 0)
    glue = _lib.FollowerGlue(None if via_a_num else d_valid.data_ptr(), d_t.data_ptr(), feedback, d_e.data_ptr(),
                             d_a.data_ptr(), d_tu.data_ptr(), d_s.data_ptr(), None, 0, None, 0, d_ce.data_ptr(),
                             d_l.data_ptr(), 0, 0, 0)
    call('sf_follower_glue_fwd', C.byref(cands), B, ptr(d_lg), C.byref(glue), stream())
    return dict(masked=down(d_lg), a=down(d_a), target_used=down(d_tu), ended=down(d_e), score=down(d_s),
                ce=down(d_ce), live=down(d_l))


@pytest.mark.parametrize('feedback', [0, 1])
@pytest.mark.parametrize('via_a_num', [False, True])
@pytest.mark.parametrize('A', [1, 2, 9, 63, 64])
def test_follower_glue_fwd_against_the_reference_lines(A, via_a_num, feedback):
    """follower.py:476-530 per row: masking (through is_valid and through a_num, every a_num of 1 .. A, the masked
    candidates holding the row's largest numbers), the first maximum (action 0 against a later action decides whether
    the agent stops), rows that had ended (target -1, no CE, still ended), targets on masked candidates (+inf CE, as
    the float64 model of the reference line gives), ignored targets."""
    case = CM.follower_glue_case(A, via_a_num)
    got = run_follower_glue(case, feedback, via_a_num)
    args = (case['logit'], case['valid'], case['target'], feedback, case['ended'])
    r, f = CM.follower_glue(*args, np.float64), CM.follower_glue(*args, F32)
    # the construction reached what it is there for
    assert set(case['a_num'].tolist()) == set(range(1, A + 1))
    alive = case['ended'] == 0
    assert (~alive).any() and alive.any()
    if A >= 9:
        assert ((case['kind'] == 1) & alive).any() and ((case['kind'] == 2) & alive).any()
        assert ((case['tkind'] == 1) & alive).any() and ((case['tkind'] == 2) & alive).any()
        assert np.isposinf(r['ce']).any()
    assert np.array_equal(bits(got['masked']), bits(r['masked']))
    for key in ('a', 'target_used', 'ended'):
        assert np.array_equal(got[key], r[key]), key
    assert np.array_equal(bits(got['live']), bits(r['live']))
    what = 'follower glue fwd A %d %s feedback %d' % (A, 'a_num' if via_a_num else 'is_valid', feedback)
    for sh in CM.SHIFTS:
        rows = case['shift'] == sh
        for key in ('score', 'ce'):
            CM.check_values('%s shift %g %s' % (what, sh, key), got[key][rows], r[key][rows], f[key][rows])
    assert not got['ce'][r['live'] == 0].any()                          # exact zeros for rows that carry no loss


# ------------------------------------------------------------------------------------------ 3. the glue, backward
def check_dlogit(what, got, r, f):
    """The gradient rule of tests/grad_compare.py, relative to the largest exact entry: e <= max(K * e32, FLOOR)."""
    scale = float(np.abs(r).max())
    if scale == 0.0:
        assert not got.any(), '%s: exact gradient zero' % what
        print('[choice] %-58s exact zero' % what)
        return
    e, e32 = float(np.abs(got - r).max()) / scale, float(np.abs(f - r).max()) / scale
    bound = max(grad_compare.K * e32, grad_compare.FLOOR)
    print('[choice] %-58s e = %.3e  e32 = %.3e  (bound %.1e, relative)' % (what, e, e32, bound))
    assert np.isfinite(got).all() and e <= bound, '%s: e = %.3e > %.3e (e32 = %.3e)' % (what, e, bound, e32)


@pytest.mark.parametrize('gscale', [0.0, 1.0, 1.0 / 7.0])
@pytest.mark.parametrize('vocab', [1, 2, 63, 64, 65, 991, 1024, 1025, 1500])
def test_speaker_glue_bwd_against_float64(vocab, gscale):
    """dlogit = gscale[0] * (softmax - onehot): rows whose target is the padding word all zero, and the padding
    COLUMNS [vocab, ldv) written zero in every row (they arrive holding poison, the logits' own hold NaN / 1e30)."""
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    for seed in range(2 if vocab == 1 else 1):
        case = CM.speaker_glue_case(vocab, seed)
        x, target, pad = case['logit'], case['target'], case['pad']
        B, ldv = len(x), ((vocab + 3) & ~3) + 4
        lg = np.empty((B, ldv), F32)
        lg[:, :vocab] = x
        lg[:, vocab:] = np.where(np.arange(ldv - vocab) % 2 == 0, np.nan, 1e30).astype(F32)
        d_lg, d_t, d_g = up(lg), up(target), up(np.array([gscale, np.nan, 1e30], F32))      # only gscale[0] is read
        d_out = up(poison_f32(B, ldv))
        call('sf_speaker_glue_bwd', B, vocab, ldv, ptr(d_lg), ptr(d_t), pad, ptr(d_g), ptr(d_out), stream())
        got = down(d_out)
        assert not bits(got[:, vocab:]).any(), 'padding columns not written zero'
        assert (pad >= vocab or (target == pad).any()) and not bits(got[target == pad]).any()
        r = CM.softmax_ce_bwd(x, target, pad, F32(gscale), np.float64)
        f = CM.softmax_ce_bwd(x, target, pad, F32(gscale), F32)
        for sh in CM.SHIFTS:
            rows = case['shift'] == sh
            check_dlogit('speaker glue bwd vocab %d gscale %.3g shift %g' % (vocab, gscale, sh), got[rows][:, :vocab],
                         r[rows], f[rows])


@pytest.mark.parametrize('gscale', [0.0, 1.0, 1.0 / 7.0])
@pytest.mark.parametrize('A', [1, 2, 9, 63, 64])
def test_follower_glue_bwd_against_float64(A, gscale):
    """The follower's entry on what its forward leaves behind: MASKED logits (-inf beyond a_num) and target_used
    (-1 for ignored and ended rows: all zero)."""
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    case = CM.follower_glue_case(A, True, seed=1)
    m = CM.follower_glue(case['logit'], case['valid'], case['target'], 0, case['ended'], np.float64)
    tused = m['target_used']                                          # (some on masked candidates: the formula still holds)
    x = m['masked']
    B = len(x)
    d_lg, d_t, d_g = up(x), up(tused), up(np.array([gscale, np.nan], F32))
    d_out = up(poison_f32(B, A))
    call('sf_follower_glue_bwd', B, A, ptr(d_lg), ptr(d_t), ptr(d_g), ptr(d_out), stream())
    got = down(d_out)
    assert (tused < 0).any() and not bits(got[tused < 0]).any()
    r = CM.softmax_ce_bwd(x, tused, -1, F32(gscale), np.float64)
    f = CM.softmax_ce_bwd(x, tused, -1, F32(gscale), F32)
    for sh in CM.SHIFTS:
        rows = case['shift'] == sh
        check_dlogit('follower glue bwd A %d gscale %.3g shift %g' % (A, gscale, sh), got[rows], r[rows], f[rows])


# ------------------------------------------------------------------------------------------------- 4. the loss
def loss_case(T, B, seed=0):
    rng = np.random.default_rng([T, B, seed])
    live = (rng.random((T, B)) < 0.6).astype(F32)
    term = (rng.random((T, B)) * 6).astype(F32) * live
    dead = np.arange(T) % 5 == 3                                       # steps with no live row ...
    live[dead] = 0
    term[dead] = 0
    term[np.arange(T) % 10 == 3] = F32(1.25)                           # ... some of which still carry a sum
    return term, live, dead


def run_reduce_finalize(term, live, T, B):
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    tail = 3
    d_term, d_live = up(term), up(live)
    d_sc, d_gs, d_loss = up(poison_f32(2 * (T + tail))), up(poison_f32(T + tail)), up(poison_f32(2))
    call('sf_reduce_terms', ptr(d_term), ptr(d_live), T, B, ptr(d_sc), stream())
    call('sf_loss_finalize', ptr(d_sc), T, ptr(d_loss), ptr(d_gs), stream())
    sc, gs, loss = down(d_sc), down(d_gs), down(d_loss)
    assert (bits(sc[2 * T:]) == POISON).all() and (bits(gs[T:]) == POISON).all() and bits(loss)[1] == POISON
    return sc[:2 * T].reshape(T, 2), gs[:T], loss[0]


def check_finalize(what, sc, gs, loss):
    """sf_loss_finalize on the float32 (sum, count) table `sc` it was given."""
    want_loss, want_gs = CM.loss_finalize(sc[:, 0], sc[:, 1])
    bound = CM.finalize_bound(sc[:, 0], sc[:, 1])
    e = abs(float(loss) - want_loss)
    print('[choice] %-58s loss %.6f  e = %.3e  (bound %.1e)' % (what, want_loss, e, bound))
    assert np.isfinite(loss) and e <= bound, (what, float(loss), want_loss, bound)
    assert np.isfinite(gs).all() and not bits(gs[sc[:, 1] <= 0]).any()            # no live row: exactly 0, not NaN
    assert (np.abs(gs - want_gs) <= 3 * CM.U32 * want_gs).all()                    # one float32 division


@pytest.mark.parametrize('B', [1, 63, 64, 65, 100, 1000])
@pytest.mark.parametrize('T', [1, 20, 64, 65, 80, 130])
def test_reduce_terms_and_loss_finalize_against_float64(T, B):
    """sum_cnt[t] = (sum_b term, sum_b live), loss = the sum over steps of the per-step means over live rows
    (test_gpu_properties.py::test_loss_is_sum_of_per_step_means_over_live_rows states it through the engine),
    gscale = 1 / count; steps without a live row add 0 and get gscale 0; T > 64 takes the kernel's second pass; the
    entries behind T stay as they were; a second run gives the same bits."""
    term, live, dead = loss_case(T, B)
    sc, gs, loss = run_reduce_finalize(term, live, T, B)
    want_sum, want_cnt = CM.reduce_terms(term, live)
    assert np.array_equal(sc[:, 1].astype(np.float64), want_cnt)                    # counts are exact
    assert (np.abs(sc[:, 0] - want_sum) <= CM.reduce_bound(term, B)).all()
    assert T < 4 or (want_cnt[dead] == 0).all() and (want_sum[dead] != 0).any()
    what = 'loss T %d B %d' % (T, B)
    check_finalize(what, sc, gs, loss)
    # the definition, from the terms themselves in float64
    steps = [t for t in range(T) if live[t].any()]
    definition = sum(float(term[t][live[t] > 0].astype(np.float64).mean()) for t in steps)
    slack = CM.finalize_bound(want_sum, want_cnt) + float((CM.reduce_bound(term, B)[steps] / want_cnt[steps]).sum())
    assert abs(float(loss) - definition) <= slack, (what, float(loss), definition, slack)
    sc2, gs2, loss2 = run_reduce_finalize(term, live, T, B)
    assert np.array_equal(bits(sc), bits(sc2)) and np.array_equal(bits(gs), bits(gs2))
    assert np.array_equal(bits(np.array([loss])), bits(np.array([loss2])))


@pytest.mark.parametrize('T', [1, 5, 64, 65, 130])
def test_loss_finalize_alone_on_a_hand_made_table(T):
    """sf_loss_finalize as after a data-parallel all-reduce: counts above any one replica's batch, and a step whose
    count is 0 while its sum is not -- it adds nothing and gets gscale 0."""
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    rng = np.random.default_rng(T)
    cnt = rng.integers(1, 8 * 1000, T).astype(F32)
    sums = (rng.random(T) * 6).astype(F32) * cnt
    zero = np.arange(T) % 4 == 0
    cnt[zero] = 0
    sums[zero] = F32(37.5)                                             # a sum without a count
    sc = np.stack([sums, cnt], 1).astype(F32)
    tail = 5
    buf = poison_f32(2 * (T + tail))
    buf[:2 * T] = sc.ravel()
    d_sc, d_gs, d_loss = up(buf), up(poison_f32(T + tail)), up(poison_f32(2))
    call('sf_loss_finalize', ptr(d_sc), T, ptr(d_loss), ptr(d_gs), stream())
    gs, loss = down(d_gs), down(d_loss)
    assert np.array_equal(bits(down(d_sc)), bits(buf))                 # its input is read only
    assert (bits(gs[T:]) == POISON).all() and bits(loss)[1] == POISON
    check_finalize('loss finalize alone T %d' % T, sc, gs[:T], loss[0])
    if T == 1:
        assert bits(loss)[0] == 0 and bits(gs)[0] == 0                 # the only step has no live row



# ------------------------------------------------------------------------- 5. the top-k order (its edges: test_gpu_search.py)
@pytest.mark.parametrize('n', [65, 991, 1024])
def test_logprob_topk_of_equal_columns_is_in_column_order(n):
    """sf_logprob_topk over rows whose best value stands in many columns -- of one thread, of one wavefront and of
    different wavefronts: the k best come lowest column first, as the beam selections take for granted (their merge
    relies on lists sorted by (value descending, column ascending))."""
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    rng = np.random.default_rng(n)
    N, k = 6, min(n, 64)
    x = (rng.standard_normal((N, n)) * 3).astype(F32)
    x[0] = F32(0.75)                                                    # a whole row equal: 0, 1, 2, ...
    for i in range(1, N):                                               # the maximum in a scattered set of columns
        x[i, rng.permutation(n)[:40]] = x[i].max() + F32(0.5)
    _, order, r, _ = CM.logprob_topk(x, None, k, np.float64)
    f = CM.logprob_topk(x, None, k, F32)[2]
    d_x = up(x)
    d_idx, d_lp = up(np.full((N, k), -7, np.int32)), up(poison_f32(N, k))
    call('sf_logprob_topk', ptr(d_x), n, N, n, None, k, ptr(d_idx), ptr(d_lp), stream())
    assert np.array_equal(down(d_idx), order)
    assert np.array_equal(order[0], np.arange(k))
    CM.check_values('logprob_topk equal columns n %d' % n, down(d_lp), r, f)


# ----------------------------------------------------------------- 6. the follower's sampled action (feedback 2) and u_next
def launch_follower_glue(logit, valid, a_num, target, ended, feedback, via_a_num, seed=0, stream_id=0, row0=0, site=None):
    """One sf_follower_glue_fwd launch without u_next on host arrays -> dict of everything it writes."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    B, A = logit.shape
    d_lg, d_t, d_e = (up(np.array(x)) for x in (logit, target, ended))    # (copies: the shared cases are read-only)
    d_valid, d_anum = up(valid.astype(F32)), up(np.array(a_num))
    d_a, d_tu = up(np.full(B, -7, np.int64)), up(np.full(B, -7, np.int64))
    d_s, d_ce, d_l = up(poison_f32(B)), up(poison_f32(B)), up(poison_f32(B))
    d_u = torch.zeros(B, A, 4, device='cuda')                         # (never read: u_next is NULL)
    d_site = None if site is None else up(np.array([site, 0x7FFFFFFF], np.int32))
    cands = _lib.Cands(d_u.data_ptr(), None, None, None, None, d_anum.data_ptr() if via_a_num else None, A, 1, 4, 0)
    glue = _lib.FollowerGlue(None if via_a_num else d_valid.data_ptr(), d_t.data_ptr(), feedback, d_e.data_ptr(),
                             d_a.data_ptr(), d_tu.data_ptr(), d_s.data_ptr(), None, 0, None, 0, d_ce.data_ptr(),
                             d_l.data_ptr(), seed, stream_id, row0, None if site is None else d_site.data_ptr())
    call('sf_follower_glue_fwd', C.byref(cands), B, ptr(d_lg), C.byref(glue), stream())
    return dict(masked=down(d_lg), a=down(d_a), target_used=down(d_tu), ended=down(d_e), score=down(d_s),
                ce=down(d_ce), live=down(d_l))


def launch_sample_case(case, via_a_num, feedback=2, rows=slice(None), stream_id=None, site=None):
    n0 = rows.start or 0
    return launch_follower_glue(case['logit'][rows], case['valid'][rows], case['a_num'][rows], case['target'][rows],
                                case['ended'][rows], feedback, via_a_num, case['seed'],
                                case['stream'] if stream_id is None else stream_id, case['row0'] + n0, site)


@functools.lru_cache(maxsize=None)
def sample_reference(A, via_a_num, special):
    case = CM.follower_sample_case(A, via_a_num, special)
    ex = CM.sample_expectation(case)
    for v in list(case.values()) + list(ex.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case, ex


@pytest.mark.parametrize('A,via_a_num,special', CM.SAMPLE_CASES)
def test_follower_glue_sample_draw_by_draw(A, via_a_num, special):
    """feedback 2 through the stand-alone kernel, every row against oracle.rng.follower_sample at the row's own uniform
    (seed, stream, row0 + b): masks with holes, every a_num, shifted rows, tails below float32's exp, rows of one
    candidate, and by row0 the global rows whose uniform is exactly 0, exactly 1 - 2^-24 and exactly 0.5 (on a row whose
    prefix sum meets u * sum exactly: `>` it is, not `>=`).  Everything else the launch
    writes is the feedback 0 launch's, bit for bit; `ended` and the score follow the action taken."""
    case, ex = sample_reference(A, via_a_num, special)
    what = 'follower glue sample A %d %s%s' % (A, 'a_num' if via_a_num else 'is_valid', ' u=' + special if special else '')
    got = launch_sample_case(case, via_a_num)
    ref = launch_sample_case(case, via_a_num, feedback=0)
    masked = np.where(case['valid'], case['logit'], F32(-np.inf)).astype(F32)
    assert np.array_equal(bits(got['masked']), bits(masked))
    share = CM.check_draws(what, got['a'], masked, case['valid'], ex)
    print('[choice] %-58s clear share %.4f, %d of %d rows' % (what, share, int(ex['clear'].sum()), len(masked)))
    assert share >= 0.99
    if special:
        at = case['at']
        assert ex['u'][at] == dict(zero=0.0, one=CM.U_ONE, half=0.5)[special]
        print('[choice] %-58s u = %.9g: action %d (mirror %d, at u (1 + 1e-5) %d)' % (what, ex['u'][at], got['a'][at],
                                                                                  ex['a'][at], ex['hi'][at]))
        # 'one': the other allowed action has float32 weight 0; 'half': every float32 operation of the row is exact
        assert got['a'][at] == ex['a'][at]
    for key in ('masked', 'target_used', 'live', 'ce'):               # the loss does not depend on the feedback
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    assert np.array_equal(got['ended'], ((case['ended'] != 0) | (got['a'] == 0)).astype(np.uint8))
    had = case['ended'] != 0
    assert A == 1 or (got['a'][had] != 0).any()                       # a row that had ended still draws
    CM.check_sample_scores(what, got['score'], masked, got['a'], case['shift'])


@pytest.mark.parametrize('name,row,valid', CM.chi2_rows(), ids=[c[0] for c in CM.chi2_rows()])
def test_follower_glue_sample_follows_softmax(name, row, valid):
    """40 000 copies of one logit row, each with its own global row id: the counts pass the chi-square test of
    test_gpu_robustness.py against float64 softmax, masked candidates are drawn exactly zero times, and every clear row
    equals the mirror (here as one searchsorted over the float64 cdf)."""
    N, A = CM.CHI2_N, len(row)
    vm = np.tile(valid, (N, 1))
    got = launch_follower_glue(np.tile(row, (N, 1)), vm, np.full(N, A, np.int32), np.zeros(N, np.int64),
                               np.zeros(N, np.uint8), 2, False, CM.SAMPLE_SEED, CM.CHI2_STREAM, CM.CHI2_ROW0)
    a = got['a']
    assert ((a >= 0) & (a < A)).all()
    counts = np.bincount(a, minlength=A).astype(np.float64)
    assert not counts[~valid].any()
    p = CM.softmax64(row, valid)
    chi2, pval = CM.chi2_softmax(counts, p, N)
    u = CM.follower_uniforms(CM.SAMPLE_SEED, CM.CHI2_STREAM, CM.CHI2_ROW0, N)
    cdf = np.cumsum(p)
    mirror = np.searchsorted(cdf / cdf[-1], u, side='right')
    clear = np.abs(cdf[valid][None, :] / cdf[-1] - u[:, None]).min(1) > CM.CLEAR
    print('[choice] follower sample chi-square %-16s chi2 = %.2f  p = %.4f  clear share %.4f' % (name, chi2, pval, clear.mean()))
    assert pval > 1e-4, (chi2, pval)
    assert clear.mean() >= 0.99 and np.array_equal(a[clear], mirror[clear])


def test_follower_glue_sample_addressing():
    """The draw is keyed on the GLOBAL row and on stream + site word: the rows [half, B) launched alone with row0 + half
    draw what they draw in the full launch; (stream s, site word k) draws what (s + k, no word) draws; two streams differ
    in at least a tenth of the rows."""
    case, ex = sample_reference(16, False, None)
    B = len(case['logit'])
    half = B // 2 + 3
    full = launch_sample_case(case, False)
    assert np.array_equal(full['a'][ex['clear']], ex['a'][ex['clear']])
    part = launch_sample_case(case, False, rows=slice(half, B))
    for key in ('a', 'ended', 'score', 'ce', 'masked'):
        assert np.array_equal(bits(part[key]), bits(full[key][half:])), key
    assert not np.array_equal(launch_follower_glue(case['logit'][half:], case['valid'][half:], case['a_num'][half:],
                                                   case['target'][half:], case['ended'][half:], 2, False, case['seed'],
                                                   case['stream'], case['row0'])['a'], full['a'][half:])
    s, k = 5, 9
    moved = launch_sample_case(case, False, stream_id=s + k)
    worded = launch_sample_case(case, False, stream_id=s, site=k)
    plain = launch_sample_case(case, False, stream_id=s)
    assert np.array_equal(worded['a'], moved['a']) and np.array_equal(bits(worded['score']), bits(moved['score']))
    assert (plain['a'] != moved['a']).mean() >= 0.1 and (plain['a'] != full['a']).mean() >= 0.1
    zero_word = launch_sample_case(case, False, stream_id=s, site=0)
    assert np.array_equal(zero_word['a'], plain['a'])


U_NEXT_B, U_NEXT_A, U_NEXT_V = 8, 5, 3
U_NEXT_SEED, U_NEXT_STREAM = 0xD1CE, 6


@pytest.mark.parametrize('feedback', [0, 1, 2])
@pytest.mark.parametrize('F4', [4, 64, 65, 544, 580])
@pytest.mark.parametrize('form', ['dense', 'fp32', 'fp16'])
def test_follower_glue_u_next_bit_for_bit(form, F4, feedback):
    """u_next[b, :F] = U[b, a_t, :F] times the mask of the NEXT step's input dropout -- site u_drop_stream + 2 * the
    u_drop site word (make_glue hands the word the multiplier 2 of the decoder's 2 * step + k numbering), global row
    u_drop.row0 + b, columns 0 .. F - 1 -- bit for bit, for dense candidates and for index-form ones on an fp32 and a
    binary16 table (zero rows for a_t = 0, a_t >= a_num and vp < 0), with u_drop absent, p = 0.5 at a non-zero row0,
    and p = 0.5 with a site word; ld_u_next = F and F + 8 with the poison behind column F untouched.  F / 4 = 580 >
    64 * 9 takes the copy loop's second pass."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    from oracle.rng import dropout_mask
    from tests import mover_cases as MC
    B, A, V = U_NEXT_B, U_NEXT_A, U_NEXT_V
    F = 4 * F4
    LOC = 0 if form == 'dense' or F4 == 4 else 16
    IMG = F - LOC
    rng = np.random.default_rng([F4, feedback, ('dense', 'fp32', 'fp16').index(form)])
    vp = np.array([0, 1, 2, -1, 0, 1, 2, 0], np.int32)
    a_num = np.array([5, 3, 1, 5, 2, 5, 4, 5], np.int32)
    target = np.array([0, 4, 0, 2, 1, 4, 3, 2], np.int64)              # teacher: stop, behind a_num, stop, vp < 0, ...
    logit = (rng.standard_normal((B, A)) * 2).astype(F32)
    logit[0, 0] = logit[0].max() + F32(40)                             # argmax and (all but surely) the sample stop in row 0
    valid = np.arange(A)[None, :] < a_num[:, None]
    cand_view = rng.integers(-1, V + 1, (B, A)).astype(np.int32)       # (clamped into the table)
    sincos = MC.sincos_constants(B * A).reshape(B, A, 4)
    if form == 'dense':
        U = (rng.standard_normal((B, A, F)) + 3).astype(F32)
        d_U, table16 = up(U), None
    else:
        table16 = MC.feature_table16(V, IMG)
        U = MC.model_candidates(table16.astype(F32), vp, cand_view, sincos, a_num, LOC)[0]
    d_vp, d_cv, d_sc, d_an = up(vp), up(cand_view), up(sincos), up(a_num)
    d_table = None if form == 'dense' else up(table16 if form == 'fp16' else table16.astype(F32))
    if d_table is not None:
        call('sf_feature_table_f16', C.c_void_p(d_table.data_ptr()), 1 if form == 'fp16' else 0)
    try:
        if form == 'dense':
            cands = _lib.Cands(d_U.data_ptr(), None, None, None, None, d_an.data_ptr(), A, 1, IMG, LOC)
        else:
            cands = _lib.Cands(None, d_table.data_ptr(), d_vp.data_ptr(), d_cv.data_ptr(), d_sc.data_ptr(), d_an.data_ptr(),
                               A, V, IMG, LOC)
        seen = set()
        for p, row0, word, ld in ((0.0, 0, None, F + 8), (0.5, 77, None, F), (0.5, 5, 3, F + 8)):
            d_lg, d_t, d_e = up(logit), up(target), up(np.zeros(B, np.uint8))
            d_a, d_tu = up(np.full(B, -7, np.int64)), up(np.full(B, -7, np.int64))
            d_s, d_ce, d_l = up(poison_f32(B)), up(poison_f32(B)), up(poison_f32(B))
            host = poison_f32(B + 1, ld)
            d_un = up(host)
            d_word = None if word is None else up(np.array([word, 0x7FFFFFFF], np.int32))
            drop = _lib.Dropout(p, U_NEXT_SEED, row0, None if word is None else d_word.data_ptr(), 0) if p else None
            glue = _lib.FollowerGlue(None, d_t.data_ptr(), feedback, d_e.data_ptr(), d_a.data_ptr(), d_tu.data_ptr(),
                                     d_s.data_ptr(), d_un.data_ptr(), ld, C.pointer(drop) if drop else None, U_NEXT_STREAM,
                                     d_ce.data_ptr(), d_l.data_ptr(), CM.SAMPLE_SEED, 2, 300, None)
            call('sf_follower_glue_fwd', C.byref(cands), B, ptr(d_lg), C.byref(glue), stream())
            a = down(d_a)
            masked = np.where(valid, logit, F32(-np.inf)).astype(F32)
            if feedback == 0:
                assert np.array_equal(a, np.maximum(target, 0))
            elif feedback == 1:
                assert np.array_equal(a, CM.first_max(masked))
            else:
                u = CM.follower_uniforms(CM.SAMPLE_SEED, 2, 300, B)
                am, margin = CM.follower_draws(masked, valid, u)
                assert (margin > CM.CLEAR).all() and np.array_equal(a, am)
            rows = U[np.arange(B), a]
            if form != 'dense':
                zero = (a == 0) | (a >= a_num) | (vp < 0)
                assert not rows[zero].any() and rows[~zero].all()
                seen |= {'stop'} if (a == 0).any() else set()
                seen |= {'behind'} if (a >= a_num).any() else set()
                seen |= {'padded'} if ((vp < 0) & (a > 0) & (a < a_num)).any() else set()
                seen |= {'row'} if (~zero).any() else set()
            mask = dropout_mask(U_NEXT_SEED, U_NEXT_STREAM + 2 * (word or 0), row0 + np.arange(B), F, p)
            want = host.copy()
            want[:B, :F] = np.where(mask != 0, rows * mask, F32(0))
            assert p == 0 or ((mask == 0).any() and (mask == 2).any())
            MC.same_bits(down(d_un), want, 'u_next %s F/4 %d feedback %d p %g row0 %d word %s ld %d' % (
                form, F4, feedback, p, row0, word, ld))
        if form != 'dense':
            assert 'row' in seen and 'stop' in seen and (feedback != 0 or seen == {'row', 'stop', 'behind', 'padded'})
    finally:
        if d_table is not None:
            torch.cuda.synchronize()
            call('sf_feature_table_f16', C.c_void_p(d_table.data_ptr()), 0)
