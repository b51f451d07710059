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
