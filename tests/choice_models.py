"""Plain numpy models of the kernels that turn numbers into a choice, and the comparison rule of their float outputs
(tests/test_gpu_choice_kernels.py, tests/test_gpu_search.py; self-tests on the CPU: tests/test_choice_models_host.py).

Every model takes the float32 array the kernel reads and a `dtype`: float64 gives the reference `r`, float32 gives `f`,
the same formula in the kernel's own precision.  Choices (arg-max, top-k order, flags) are made on the float32 values
themselves -- the lowest index among the maxima -- so they do not depend on `dtype`.

    speaker_glue / follower_glue     speaker.py:163-191 / follower.py:476-530 per row
    softmax_ce_bwd                   gscale * (softmax - onehot), zero rows for ignored targets
    reduce_terms / loss_finalize     per-step (sum, count), the sum of per-step means, 1 / count
    logprob_topk                     masked log-softmax and the stable descending order of the masked row
"""
import numpy as np

from tests.grad_compare import K

F32 = np.float32
FLOOR = 1e-5                     # the atol of this quantity in test_gpu_search.py::test_logprob_topk_kernel_against_torch
U32 = 2.0 ** -24                 # unit roundoff of float32


def lse(x, dtype):
    """log-sum-exp of the last axis in `dtype`; -inf entries count as zero probability (at least one finite entry)."""
    x = np.asarray(x, dtype)
    m = x.max(-1)
    with np.errstate(divide='ignore'):
        return (m + np.log(np.exp(x - m[..., None]).sum(-1, dtype=dtype)).astype(dtype)).astype(dtype)


def first_max(x):
    """torch.max semantics: the lowest index among the maxima of every row (np.argmax returns the first one)."""
    return np.argmax(x, -1).astype(np.int64)


def speaker_glue(logit, target, feedback, pad, eos, ended, dtype):
    """logit float32 [B, vocab]; target int64 [B]; feedback 0 teacher / 1 argmax; ended uint8 [B] before the step."""
    assert logit.dtype == F32 and feedback in (0, 1)
    B = len(logit)
    rows = np.arange(B)
    z = lse(logit, dtype)
    x = logit.astype(dtype)
    w = target.astype(np.int64) if feedback == 0 else first_max(logit)
    score = np.where(w != pad, x[rows, w] - z, 0).astype(dtype)              # speaker.py:179-180
    lv = target != pad
    nll = np.where(lv, z - x[rows, target], 0).astype(dtype)                 # speaker.py:182, per row
    out_ended = ended.copy()
    out_ended[w == eos] = 1                                                  # speaker.py:190-191
    return dict(w=w, ended=out_ended, score=score, nll=nll, live=lv.astype(F32))


def follower_glue(logit, valid, target, feedback, ended, dtype):
    """logit float32 [B, A]; valid bool [B, A]; target int64 [B] (-1 = ignore); ended uint8 [B] before the step."""
    assert logit.dtype == F32 and feedback in (0, 1)
    B = len(logit)
    rows = np.arange(B)
    masked = np.where(valid, logit, F32(-np.inf)).astype(F32)                # follower.py:477
    z = lse(masked, dtype)
    x = masked.astype(dtype)
    tgt = np.where(ended != 0, -1, target).astype(np.int64)                  # follower.py:322-328
    live = tgt >= 0
    ce = np.where(live, z - x[rows, np.maximum(tgt, 0)], 0).astype(dtype)    # CrossEntropyLoss(ignore_index=-1)
    a = np.maximum(tgt, 0) if feedback == 0 else first_max(masked)           # follower.py:486 / 488
    score = (x[rows, a] - z).astype(dtype)                                   # follower.py:504
    out_ended = ((ended != 0) | (a == 0)).astype(np.uint8)                   # follower.py:527-530
    return dict(masked=masked, a=a, target_used=tgt, ended=out_ended, score=score, ce=ce, live=live.astype(F32))


def softmax_ce_bwd(logit, target, ignore, gscale, dtype):
    """gscale * (softmax(logit) - onehot(target)) per row of logit float32 [B, N]; rows with target == ignore: zeros."""
    assert logit.dtype == F32
    x = logit.astype(dtype)
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True, dtype=dtype)
    keep = target != ignore
    p[np.flatnonzero(keep), target[keep]] -= dtype(1)
    return (dtype(gscale) * p * keep[:, None]).astype(dtype)


def reduce_terms(term, live):
    """term, live float32 [T, B] -> (sum [T], count [T]) in float64."""
    return term.astype(np.float64).sum(1), live.astype(np.float64).sum(1)


def loss_finalize(sums, counts):
    """(loss, gscale [T]) in float64 from per-step sums and counts: steps without a live row add 0 and get gscale 0."""
    s, c = np.asarray(sums, np.float64), np.asarray(counts, np.float64)
    on = c > 0
    safe = np.where(on, c, 1.0)
    return float(np.where(on, s / safe, 0.0).sum()), np.where(on, 1.0 / safe, 0.0)


def reduce_bound(term, B):
    """A priori bound of sf_reduce_terms' float32 sum per step: every lane adds ceil(B / 64) terms one after the other,
    the 64 lane sums meet in a 6-level tree, so each term passes through at most d = ceil(B / 64) + 6 roundings and
    |got - exact| <= ((1 + u)^d - 1) * sum |term| <= 1.01 d u sum |term|."""
    d = -(-B // 64) + 6
    return 1.01 * d * U32 * np.abs(term.astype(np.float64)).sum(1)


def finalize_bound(sums, counts):
    """A priori bound of sf_loss_finalize's loss: one float32 division per step (at most 2.5 ulp < 3 u relative, the
    bound of HIP's float32 division when it is not correctly rounded) and T - 1 additions in step order, so
    |got - exact| <= 1.01 (T + 2) u sum_t |mean_t|."""
    s, c = np.asarray(sums, np.float64), np.asarray(counts, np.float64)
    mean = np.where(c > 0, np.abs(s) / np.where(c > 0, c, 1.0), 0.0)
    return 1.01 * (len(s) + 2) * U32 * float(mean.sum())


def logprob_topk(logit, n_valid, k, dtype):
    """logit float32 [N, n]; n_valid int [N] or None.  Returns (masked float32 [N, n], idx [N, k], logp [N, k], logp of
    the whole row in column order [N, n]): columns >= n_valid are -inf, the order is the stable descending sort of the
    masked row -- so once the finite columns run out the -inf columns, masked or not, follow in column order."""
    assert logit.dtype == F32
    N, n = logit.shape
    masked = logit.copy()
    if n_valid is not None:
        masked[np.arange(n)[None, :] >= np.asarray(n_valid)[:, None]] = -np.inf
    with np.errstate(invalid='ignore'):
        lp = (masked.astype(dtype) - lse(masked, dtype)[:, None]).astype(dtype)
    lp[np.isneginf(masked)] = -np.inf
    order = np.stack([np.lexsort((np.arange(n), -masked[i].astype(np.float64))) for i in range(N)])[:, :k]
    return masked, order.astype(np.int32), np.take_along_axis(lp, order, 1), lp


def check_values(what, got, r, f, floor=FLOOR, k=K):
    """The project's rule for float outputs (tests/grad_compare.py): with r the float64 model and f the same formula
    in float32, e = max|got - r| must satisfy e <= max(K * max|f - r|, floor).  Non-finite entries of r (the -inf of a
    masked candidate, the +inf of a target on one) must be the same non-finite value in `got`.  Prints e and e32."""
    got, r, f = np.asarray(got, np.float64), np.asarray(r, np.float64), np.asarray(f, np.float64)
    assert got.shape == r.shape == f.shape, (what, got.shape, r.shape, f.shape)
    fin = np.isfinite(r)
    assert np.array_equal(np.isfinite(got), fin), '%s: the finite / non-finite pattern differs' % what
    assert np.array_equal(got[~fin], r[~fin]), '%s: non-finite values differ' % what
    e = float(np.abs(got[fin] - r[fin]).max()) if fin.any() else 0.0
    e32 = float(np.abs(f[fin] - r[fin]).max()) if fin.any() else 0.0
    bound = max(k * e32, floor)
    print('[choice] %-58s e = %.3e  e32 = %.3e  (bound %.1e)' % (what, e, e32, bound))
    assert e <= bound, '%s: e = %.3e > max(%g x e32 %.3e, %.0e)' % (what, e, k, e32, floor)
    return e, e32


# ------------------------------------------------------------------------------------------------ constructed inputs
GAP = F32(2.0 ** -9)             # >= 1e-3, and two float32 steps at 1e4: the runner-up of a row without a tie
SHIFTS = (0.0, 80.0, -80.0, 1e4)


def shifted_rows(rng, B, n, shifts=SHIFTS):
    """Rows of logits, row i moved by shifts[i % len] BEFORE it is rounded to float32: kernel and models read the same
    float32 numbers."""
    sh = np.asarray(shifts, np.float64)[np.arange(B) % len(shifts)]
    return (rng.standard_normal((B, n)) * 3.0 + sh[:, None]).astype(F32), sh


def raise_columns(x, i, cols, among=None):
    """Make `cols` the (equal) maxima of row i of float32 x, GAP above every other column of `among` (default: all)."""
    among = np.arange(x.shape[1]) if among is None else np.asarray(among)
    rest = np.setdiff1d(among, cols)
    top = x[i, rest].max() if len(rest) else x[i, cols].max()
    x[i, cols] = F32(top + GAP * F32(1 + i % 3))
    assert len(rest) == 0 or x[i, cols[0]] - x[i, rest].max() >= 1e-3


def speaker_tie_pairs(vocab):
    """Column pairs that hold the duplicated maximum: neighbouring lanes, one lane's own columns, first / last column,
    the boundary between the register path (columns < 1024) and the loop behind it."""
    pairs = [(c, c + 1) for c in (0, 30, 63, vocab - 2) if 0 <= c and c + 1 < vocab]
    pairs += [(c, c + 64) for c in (0, 17, vocab - 65) if 0 <= c and c + 64 < vocab]
    pairs += [(0, vocab - 1)] if vocab > 1 else []
    if vocab > 1024:
        pairs += [(1023, 1024), (0, 1024), (5, vocab - 1)] + ([(1024, vocab - 1)] if vocab > 1025 else [])
        pairs += [(1024, 1088)] if vocab > 1088 else []            # one lane's own columns, both behind 1024
    return sorted(set(pairs))


def speaker_glue_case(vocab, seed=0):
    """Inputs of one sf_speaker_glue_fwd / _bwd case: dict(logit [B, vocab] float32, target, pad, eos, ended, kinds)."""
    rng = np.random.default_rng(1000 + vocab + seed)
    pad, eos = (0, 2) if vocab >= 3 else ((0, 1) if vocab == 2 else ((0, 7) if seed % 2 == 0 else (7, 0)))
    pairs = speaker_tie_pairs(vocab)
    B = 4 * 3 * max(2 * len(pairs), 4)
    x, sh = shifted_rows(rng, B, vocab)
    target = rng.integers(0, vocab, B)
    tie = np.zeros(B, bool)
    best = np.zeros(B, np.int64)
    for i in range(B):
        kind = (i // 4) % 3                                     # the target: ordinary, pad, EOS (where the vocabulary has it)
        if kind == 1 and pad < vocab:
            target[i] = pad
        if kind == 2 and eos < vocab:
            target[i] = eos
        j = i // 12
        if j % 2 == 0 and pairs:                                # a duplicated maximum
            cols = np.array(pairs[(j // 2) % len(pairs)])
            tie[i] = True
        else:                                                   # one maximum, GAP clear of the rest; EOS now and then
            cols = np.array([eos if (j % 4 == 1 and eos < vocab) else int(rng.integers(0, vocab))])
        raise_columns(x, i, cols)
        best[i] = cols.min()
    ended = np.where(rng.random(B) < 0.5, 0, np.where(rng.random(B) < 0.5, 1, 0xA5)).astype(np.uint8)
    return dict(logit=x, shift=sh, target=target.astype(np.int64), pad=pad, eos=eos, ended=ended, tie=tie, best=best)


def follower_glue_case(A, via_a_num, seed=0):
    """Inputs of one sf_follower_glue_fwd / _bwd case: every a_num of 1 .. A, rows that had ended, ties between action
    0 and a later action and between two later actions, targets on valid and on masked candidates and ignored ones."""
    rng = np.random.default_rng(2000 + 10 * A + seed + (5 if via_a_num else 0))
    B = 4 * max(A, 24)
    x, sh = shifted_rows(rng, B, A)
    a_num = 1 + rng.permutation(B) % A
    valid = np.arange(A)[None, :] < a_num[:, None]
    target = np.zeros(B, np.int64)
    ended = (rng.random(B) < 0.25).astype(np.uint8)
    kind = np.zeros(B, np.int64)                                # 0 one maximum, 1 action 0 ties a later one, 2 two later tie
    tkind = np.zeros(B, np.int64)                               # 0 valid target, 1 masked target, 2 ignored
    for i in range(B):
        n = int(a_num[i])
        want = int(rng.integers(0, 3))
        if want == 1 and n >= 2:
            cols = np.array([0, int(rng.integers(1, n))])
        elif want == 2 and n >= 3:
            cols = np.sort(rng.choice(np.arange(1, n), 2, replace=False))
        else:
            want, cols = 0, np.array([int(rng.integers(0, n))])
        kind[i] = want
        raise_columns(x, i, cols, among=np.arange(n))
        x[i, n:] = x[i, cols[0]] + F32(1 + 7 * rng.random())    # masked candidates score ABOVE every valid one
        tk = int(rng.integers(0, 4))
        if tk == 1 and n < A:
            tkind[i], target[i] = 1, int(rng.integers(n, A))
        elif tk == 2:
            tkind[i], target[i] = 2, -1
        else:
            target[i] = int(rng.integers(0, n))
    return dict(logit=x, shift=sh, a_num=a_num.astype(np.int32), valid=valid, target=target, ended=ended, kind=kind,
                tkind=tkind)
