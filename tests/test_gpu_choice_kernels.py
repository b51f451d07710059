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

The shifted rows cost what float32 costs there -- one step of a logit near 1e4 is 9.8e-04 -- and the kernels stay within
the float32 model's own error.  The whole module (131 tests) takes 4 to 5 s of wall time, 0.5 s of it in its slowest test
(the beam selection at B = 64, beam 64).
"""
import ctypes as C
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
