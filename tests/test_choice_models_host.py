"""CPU: the numpy models of tests/choice_models.py against torch's own float64 operators -- the models are the yardstick
of tests/test_gpu_choice_kernels.py, so they are checked here against an independent statement of the same lines
(torch.max, F.log_softmax, F.nll_loss, F.cross_entropy, autograd, a stable sort)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import choice_models as CM

F32 = np.float32


def rows(seed, B, n, shift=0.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, n)) * 3 + shift).astype(F32)


@pytest.mark.parametrize('vocab,shift', [(1, 0.0), (2, 80.0), (65, -80.0), (991, 0.0), (1500, 1e4)])
def test_speaker_glue_model_is_the_reference_lines(vocab, shift):
    B, pad, eos = 24, 0, min(2, vocab - 1)
    x = rows(vocab, B, vocab, shift)
    x[1, vocab // 2:] = x[1].max() + F32(1)                       # a run of equal maxima: the first one wins
    rng = np.random.default_rng(1)
    target = rng.integers(0, vocab, B)
    target[:3] = pad, eos, vocab - 1
    ended = (rng.random(B) < 0.3).astype(np.uint8)
    t = torch.tensor(x, dtype=torch.float64)
    lp = F.log_softmax(t, dim=1)
    for feedback in (0, 1):
        m = CM.speaker_glue(x, target, feedback, pad, eos, ended, np.float64)
        w = torch.tensor(target) if feedback == 0 else t.max(1)[1]
        assert np.array_equal(m['w'], w.numpy())
        score = -F.nll_loss(lp, w, ignore_index=pad, reduction='none')
        nll = F.nll_loss(lp, torch.tensor(target), ignore_index=pad, reduction='none')
        np.testing.assert_allclose(m['score'], score.numpy(), rtol=0, atol=1e-9)
        np.testing.assert_allclose(m['nll'], nll.numpy(), rtol=0, atol=1e-9)
        assert np.array_equal(m['live'], (target != pad).astype(F32))
        assert np.array_equal(m['ended'], np.where(w.numpy() == eos, 1, ended))
        f = CM.speaker_glue(x, target, feedback, pad, eos, ended, F32)
        assert f['score'].dtype == F32 and np.array_equal(f['w'], m['w'])
        assert np.abs(f['score'] - m['score']).max() <= 4e-7 * max(1.0, abs(shift)) * 8


@pytest.mark.parametrize('A', [1, 2, 9, 64])
def test_follower_glue_model_is_the_reference_lines(A):
    B = 40
    rng = np.random.default_rng(A)
    x = rows(A + 7, B, A)
    a_num = rng.integers(1, A + 1, B)
    valid = np.arange(A)[None, :] < a_num[:, None]
    target = rng.integers(-1, A, B)                                # some ignored, some on a masked candidate
    ended = (rng.random(B) < 0.3).astype(np.uint8)
    x[0, :] = x[0].max()                                           # every candidate equal: action 0, the row ends
    t = torch.tensor(x, dtype=torch.float64)
    t[torch.tensor(~valid)] = -float('inf')
    tgt = torch.tensor(np.where(ended != 0, -1, target))
    ce = F.cross_entropy(t, tgt, ignore_index=-1, reduction='none')
    for feedback in (0, 1):
        m = CM.follower_glue(x, valid, target, feedback, ended, np.float64)
        a = torch.clamp(tgt, min=0) if feedback == 0 else t.max(1)[1]
        assert np.array_equal(m['a'], a.numpy()) and np.array_equal(m['target_used'], tgt.numpy())
        score = -F.cross_entropy(t, a, ignore_index=-1, reduction='none')
        for got, want in ((m['ce'], ce.numpy()), (m['score'], score.numpy())):
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
            np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=1e-9)
        assert np.array_equal(m['ended'], ((ended != 0) | (a.numpy() == 0)).astype(np.uint8))
        assert np.array_equal(m['live'], (tgt.numpy() >= 0).astype(F32))
        assert np.array_equal(m['masked'], t.numpy().astype(F32))
    assert m['a'][0] == 0 and m['ended'][0] == 1


@pytest.mark.parametrize('n,ignore', [(1, -1), (9, -1), (64, -1), (991, 0), (1500, 0)])
def test_softmax_ce_bwd_model_is_autograd_of_the_summed_loss(n, ignore):
    B, gs = 12, 1.0 / 7.0
    x = rows(n, B, n)
    target = np.random.default_rng(n).integers(0, n, B)
    target[::4] = ignore if ignore >= 0 else -1
    if ignore < 0:
        x[1, n // 2:] = -np.inf if n > 1 else x[1, 0]              # masked candidates (never the target's)
        target[1] = 0
    t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (gs * F.cross_entropy(t, torch.tensor(target), ignore_index=ignore, reduction='sum')).backward()
    m = CM.softmax_ce_bwd(x, target, ignore, gs, np.float64)
    np.testing.assert_allclose(m, t.grad.numpy(), rtol=0, atol=1e-12)
    assert not m[::4].any()


def test_loss_model_is_the_sum_of_per_step_means_over_live_rows():
    rng = np.random.default_rng(0)
    T, B = 9, 13
    live = (rng.random((T, B)) < 0.6).astype(F32)
    live[3] = 0
    term = (rng.random((T, B)) * 5).astype(F32) * live
    s, c = CM.reduce_terms(term, live)
    loss, gscale = CM.loss_finalize(s, c)
    want = sum(float(term[t][live[t] > 0].astype(np.float64).mean()) for t in range(T) if live[t].any())
    assert abs(loss - want) < 1e-12 and gscale[3] == 0 and np.allclose(gscale[c > 0], 1 / c[c > 0])
    assert CM.loss_finalize([5.0, 2.0], [0.0, 4.0]) [0] == 0.5     # a sum without a count adds nothing


def test_topk_model_is_a_stable_descending_sort_of_the_masked_row():
    rng = np.random.default_rng(2)
    N, n, k = 6, 37, 37
    x = rows(3, N, n)
    x[:, 5] = x[:, 2]
    x[0] = F32(1.5)                                                # a whole row equal: 0, 1, 2, ...
    x[1, [0, 3, 4]] = -np.inf                                      # valid columns that are -inf
    nv = rng.integers(6, n + 1, N)
    masked, idx, logp, rowlp = CM.logprob_topk(x, nv, k, np.float64)
    t = torch.tensor(x, dtype=torch.float64)
    t[torch.arange(n)[None, :] >= torch.tensor(nv)[:, None]] = -float('inf')
    order = torch.sort(t, dim=1, descending=True, stable=True)[1]
    assert np.array_equal(idx, order.numpy()) and np.array_equal(masked, t.numpy().astype(F32))
    lp = torch.log_softmax(t, 1)
    fin = np.isfinite(lp.numpy())
    assert np.array_equal(np.isfinite(rowlp), fin)
    np.testing.assert_allclose(rowlp[fin], lp.numpy()[fin], rtol=0, atol=1e-9)
    assert np.array_equal(idx[0, :nv[0]], np.arange(nv[0]))
    assert np.array_equal(logp, np.take_along_axis(rowlp, idx.astype(np.int64), 1))


def test_check_values_holds_the_rule():
    r = np.array([1.0, 2.0, -np.inf])
    f = r + np.array([1e-5, 0, 0])
    CM.check_values('inside', r + np.array([0, 3.9e-5, 0]), r, f)
    with pytest.raises(AssertionError):
        CM.check_values('outside', r + np.array([0, 4.1e-5, 0]), r, f)
    with pytest.raises(AssertionError):
        CM.check_values('pattern', np.array([1.0, 2.0, 0.0]), r, f)
    with pytest.raises(AssertionError):
        CM.check_values('floor', r + np.array([0, 1.1e-5, 0]), r, r)
    CM.check_values('floor', r + np.array([0, 0.9e-5, 0]), r, r)


# ------------------------------------------------------------------------------- the follower's sampled action (mirror)
def test_the_planted_uniforms_are_exactly_zero_and_one_minus_ulp():
    """The two global rows tests/choice_models.py places by row0, from the generator itself; and the site word adds to
    the stream (sf_glue.h: seed + G * site, then dropout_row_key adds G * stream)."""
    from oracle.rng import sample_uniforms, dropout_bits
    z, o = CM.U_ZERO_AT, CM.U_ONE_AT
    assert sample_uniforms(z['seed'], z['stream'], [z['row']])[0][0] == 0.0
    assert sample_uniforms(o['seed'], o['stream'], [o['row']])[0][0] == CM.U_ONE == 1.0 - 2.0 ** -24
    h = CM.U_HALF_AT
    assert sample_uniforms(h['seed'], h['stream'], [h['row']])[0][0] == 0.5
    rows = np.arange(50) + 300
    G = 0x9E3779B9
    for seed, stream, site in ((CM.SAMPLE_SEED, 3, 5), (0xFFFFFFF0, 0xFFFFFFFE, 7)):
        moved = dropout_bits((seed + G * site) & 0xFFFFFFFF, stream, rows, [0])
        assert np.array_equal(moved, dropout_bits(seed, (stream + site) & 0xFFFFFFFF, rows, [0]))
    u = CM.follower_uniforms(CM.SAMPLE_SEED, 1, z['row'] - 7, 9)
    assert u[7] == 0.0 and ((u >= 0) & (u < 1)).all() and len(set(u)) == 9


def brute_force_draw(masked, valid, u):
    """The same draw by searchsorted over the valid candidates only."""
    v = np.flatnonzero(valid)
    l = masked[v].astype(np.float64)
    cdf = np.cumsum(np.exp(l - l.max()))
    k = int(np.searchsorted(cdf, u * cdf[-1], side='right'))         # the first cdf strictly above the threshold
    return int(v[min(k, len(v) - 1)]), float(np.abs(cdf - u * cdf[-1]).min() / cdf[-1])


@pytest.mark.parametrize('A,via_a_num,special', CM.SAMPLE_CASES)
def test_follower_sample_mirror_is_searchsorted_and_the_cases_are_clear(A, via_a_num, special):
    """oracle.rng.follower_sample against the brute-force formulation on every row of every launch of
    test_gpu_choice_kernels.py section 6; the share of clear draws there is at least 0.99; the row kinds the builder
    promises are present."""
    case = CM.follower_sample_case(A, via_a_num, special)
    ex = CM.sample_expectation(case)
    masked = np.where(case['valid'], case['logit'], F32(-np.inf)).astype(F32)
    for i in range(len(masked)):
        a, m = brute_force_draw(masked[i], case['valid'][i], ex['u'][i])
        assert a == ex['a'][i] and abs(m - ex['margin'][i]) <= 1e-15, i
        assert case['valid'][i, ex['a'][i]] and case['valid'][i, ex['lo'][i]] and case['valid'][i, ex['hi'][i]]
    assert ex['clear'].mean() >= 0.99, ex['clear'].mean()
    n_valid = case['valid'].sum(1)
    assert (n_valid >= 1).all() and (n_valid == 1).any()
    if via_a_num:
        assert set(case['a_num'].tolist()) == set(range(1, A + 1))
        assert np.array_equal(case['valid'], np.arange(A)[None, :] < case['a_num'][:, None])
    elif A >= 9:
        assert set(case['hole'].tolist()) == {0, 1, 2, 3}
        h1 = np.flatnonzero(case['hole'] == 1)[0]
        inv = np.flatnonzero(~case['valid'][h1, :case['a_num'][h1]])
        assert len(inv) == 1 and case['valid'][h1, :inv[0]].any() and case['valid'][h1, inv[0] + 1:].any()
        assert (~case['valid'][case['hole'] == 2, 0]).all()
        last = case['valid'][case['hole'] == 3]
        assert last[:, -1].all() and (last.sum(1) == 1).all()
    assert set(case['shift'].tolist()) == set(CM.SHIFTS)
    if A >= 2:
        assert case['wide'].any()
        for i in np.flatnonzero(case['wide']):
            l = masked[i][case['valid'][i]]
            assert l.max() - l.min() > CM.UNDERFLOW
            assert (np.exp((l - l.max()).astype(F32)) == 0).any()          # float32's exp is 0 on the tail
    assert len(set(ex['a'].tolist())) > 1 or A == 1
    if special == 'zero':
        at = case['at']
        first = int(np.flatnonzero(case['valid'][at])[0])
        assert ex['u'][at] == 0.0 and ex['a'][at] == first and ex['clear'][at]
        assert first == (0 if via_a_num else 1)
    if special == 'half':
        at = case['at']
        e = np.exp((masked[at] - masked[at].max()).astype(F32))
        assert ex['u'][at] == 0.5 and e.sum() == 2 and set(e.tolist()) <= {0.0, 1.0}
        assert ex['margin'][at] == 0 and (ex['lo'][at], ex['a'][at], ex['hi'][at]) == ((A - 1) // 2, A - 1, A - 1)
    if special == 'one':
        at = case['at']
        assert ex['u'][at] == CM.U_ONE and not ex['clear'][at]
        # the mirror never takes a candidate of the underflowing tail; at u * (1 + CLEAR) > 1 it falls back to the last one
        head = (A + 1) // 2
        assert ex['a'][at] < head and ex['hi'][at] == A - 1
        assert case['zero_pick'] == (A >= 9)                               # (A = 2: one weight, the sums are exact)


def test_follower_glue_model_under_sampling():
    """feedback 2 of CM.follower_glue: the action is the mirror's, score = log p(action) by torch's float64
    log_softmax, the loss side is the teacher's, and a row that had ended still draws and ends on action 0."""
    case = CM.follower_sample_case(9, False)
    ex = CM.sample_expectation(case)
    args = (case['logit'], case['valid'], case['target'])
    m = CM.follower_glue(*args, 2, case['ended'], np.float64, u=ex['u'])
    t0 = CM.follower_glue(*args, 0, case['ended'], np.float64)
    assert np.array_equal(m['a'], ex['a'])
    for key in ('masked', 'target_used', 'live'):
        assert np.array_equal(m[key], t0[key])
    assert np.array_equal(np.isfinite(m['ce']), np.isfinite(t0['ce'])) and np.array_equal(m['ce'], t0['ce'])
    lp = F.log_softmax(torch.tensor(m['masked'], dtype=torch.float64), dim=1).numpy()
    np.testing.assert_allclose(m['score'], lp[np.arange(len(lp)), m['a']], rtol=0, atol=1e-9)
    assert np.isfinite(m['score']).all()
    assert np.array_equal(m['ended'], ((case['ended'] != 0) | (m['a'] == 0)).astype(np.uint8))
    had = case['ended'] != 0
    assert (m['a'][had] != 0).any() and len(set(m['a'][had].tolist())) > 1
    with pytest.raises(AssertionError):
        CM.follower_glue(*args, 2, case['ended'], np.float64)


@pytest.mark.parametrize('name,row,valid', CM.chi2_rows(), ids=[c[0] for c in CM.chi2_rows()])
def test_the_mirror_itself_follows_softmax(name, row, valid):
    """The chi-square test of test_gpu_choice_kernels.py on the mirror's own draws, at the same seed, stream and rows:
    what the device is held to is met by the float64 statement of it."""
    N = CM.CHI2_N
    u = CM.follower_uniforms(CM.SAMPLE_SEED, CM.CHI2_STREAM, CM.CHI2_ROW0, N)
    p = CM.softmax64(row, valid)
    cdf = np.cumsum(p)
    a = np.searchsorted(cdf / cdf[-1], u, side='right')
    spot = np.arange(0, N, 97)
    masked = np.where(valid, row, F32(-np.inf)).astype(F32)
    assert np.array_equal(a[spot], CM.follower_draws(np.tile(masked, (len(spot), 1)), np.tile(valid, (len(spot), 1)), u[spot])[0])
    counts = np.bincount(a, minlength=len(row)).astype(np.float64)
    assert not counts[~valid].any()
    chi2, pval = CM.chi2_softmax(counts, p, N)
    print('[choice] mirror chi-square %-16s chi2 = %.2f  p = %.4f' % (name, chi2, pval))
    assert pval > 1e-4, (chi2, pval)
    margin = np.abs(cdf[valid][None, :] / cdf[-1] - u[:, None]).min(1)
    assert (margin > CM.CLEAR).mean() >= 0.99


def test_f32_lane_sums_is_a_scan_and_a_sum():
    e = np.random.default_rng(0).random(37).astype(F32)
    cdf, se = CM.f32_lane_sums(e)
    np.testing.assert_allclose(cdf[:37], np.cumsum(e.astype(np.float64)), rtol=1e-6)
    assert abs(float(se) - float(e.astype(np.float64).sum())) <= 1e-6 * float(se)
    np.testing.assert_allclose(cdf[37:], cdf[36], rtol=1e-6)          # (level up to rounding: each lane adds in its own order)
    cdf, se = CM.f32_lane_sums(np.ones(64, F32))
    assert np.array_equal(cdf, np.arange(1, 65, dtype=F32)) and se == 64
