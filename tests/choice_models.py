"""Plain numpy models of the kernels that turn numbers into a choice, and the comparison rule of their float outputs
(tests/test_gpu_choice_kernels.py, tests/test_gpu_search.py; self-tests on the CPU: tests/test_choice_models_host.py).

Every model takes the float32 array the kernel reads and a `dtype`: float64 gives the reference `r`, float32 gives `f`,
the same formula in the kernel's own precision.  Choices (arg-max, top-k order, flags) are made on the float32 values
themselves -- the lowest index among the maxima -- so they do not depend on `dtype`.

    speaker_glue / follower_glue     speaker.py:163-191 / follower.py:476-530 per row
    softmax_ce_bwd                   gscale * (softmax - onehot), zero rows for ignored targets
    reduce_terms / loss_finalize     per-step (sum, count), the sum of per-step means, 1 / count
    logprob_topk                     masked log-softmax and the stable descending order of the masked row
    follower_glue(feedback=2, u=)    the sampled action: oracle.rng.follower_sample at the row's uniform, always in float64
    follower_sample_case, sample_expectation, check_draws, check_sample_scores, chi2_softmax
                                     the launches of test_gpu_choice_kernels.py section 6, the mirror's side of each, the
                                     draw-by-draw rule and the chi-square test (also used by test_gpu_follower_sample.py)
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


def follower_draws(masked, valid, u, eps=0.0):
    """oracle.rng.follower_sample per row at the uniforms u * (1 + eps) -> (action int64 [B], margin float64 [B])."""
    from oracle.rng import follower_sample
    out = [follower_sample(masked[i], valid[i], float(u[i]) * (1.0 + eps)) for i in range(len(masked))]
    return np.array([a for a, _ in out], np.int64), np.array([m for _, m in out], np.float64)


def follower_glue(logit, valid, target, feedback, ended, dtype, u=None):
    """logit float32 [B, A]; valid bool [B, A]; target int64 [B] (-1 = ignore); ended uint8 [B] before the step;
    feedback 0 teacher / 1 argmax / 2 sample with the uniforms u float64 [B] (oracle.rng.follower_sample: the draw is
    made in float64 whatever `dtype` is, and a row that had ended draws like any other)."""
    assert logit.dtype == F32 and feedback in (0, 1, 2) and (feedback == 2) == (u is not None)
    B = len(logit)
    rows = np.arange(B)
    masked = np.where(valid, logit, F32(-np.inf)).astype(F32)                # follower.py:477
    z = lse(masked, dtype)
    x = masked.astype(dtype)
    tgt = np.where(ended != 0, -1, target).astype(np.int64)                  # follower.py:322-328
    live = tgt >= 0
    ce = np.where(live, z - x[rows, np.maximum(tgt, 0)], 0).astype(dtype)    # CrossEntropyLoss(ignore_index=-1)
    if feedback == 2:
        a = follower_draws(masked, valid, u)[0]                              # follower.py:491-497
    else:
        a = np.maximum(tgt, 0) if feedback == 0 else first_max(masked)       # follower.py:486 / 488
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


# ----------------------------------------------------------------------------------- the follower's sampled action
SAMPLE_SEED = 0xC0FFEE
CLEAR = 1e-5                     # a draw whose margin (oracle.rng.follower_sample) exceeds this is out of float32's reach
U_ONE = 1.0 - 2.0 ** -24         # the largest uniform the device forms: (2^24 - 1) / 2^24
# global rows whose uniform at (SAMPLE_SEED, stream 1) is exactly 0 / exactly U_ONE (found by a scan of oracle.rng's
# sample_uniforms over row ids; tests/test_choice_models_host.py re-verifies both)
U_ZERO_AT = dict(seed=SAMPLE_SEED, stream=1, row=7078075)
U_ONE_AT = dict(seed=SAMPLE_SEED, stream=1, row=25335644)
U_HALF_AT = dict(seed=SAMPLE_SEED, stream=1, row=7127063)      # ... and exactly 0.5
UNDERFLOW = 104.0                # expf(-x) is 0 in float32 for x > 103.98 (flushed) .. 104 (rounded)


def follower_uniforms(seed, stream, row0, B):
    """The uniforms of rows row0 .. row0 + B - 1 at (seed, stream): sf_glue.h keys the draw of row b on
    dropout_row_key(seed + G * site, stream, row0 + b) = the key of stream + site, and takes the top 24 bits of the
    hash of column 0 -- sample_uniforms(...)[0]."""
    from oracle.rng import sample_uniforms
    return sample_uniforms(seed, stream, np.arange(B, dtype=np.int64) + row0)[0]


def softmax64(row, valid=None):
    x = np.asarray(row, np.float64)
    e = np.exp(x - x[valid if valid is not None else slice(None)].max())
    if valid is not None:
        e = np.where(valid, e, 0.0)
    return e / e.sum()


def chi2_softmax(counts, p, n):
    """The chi-square test of tests/test_gpu_robustness._chi2: cells with p * n < 5 are pooled into one (and that one
    into its neighbour while it is still below 5) -> (chi2, p-value); callers assert p-value > 1e-4."""
    from scipy import stats
    keep = p * n >= 5
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(p[keep] * n, p[~keep].sum() * n)
    if exp[-1] < 5:
        obs[-2] += obs[-1]
        exp[-2] += exp[-1]
        obs, exp = obs[:-1], exp[:-1]
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    return chi2, float(stats.chi2.sf(chi2, len(obs) - 1))


def f32_lane_sums(e):
    """What the glue's two float32 sums over 64 lanes make of the weights e [<= 64]: (the inclusive shuffle-up scan's
    value in every lane, the butterfly sum).  Every lane's additions come in an order of their own, so over a run of zero
    weights the scan need not stay level, and its last value can stand below the butterfly's sum.  Used to BUILD rows
    on which that matters (numpy's
    float32 exp may differ from the device's by an ulp, so this predicts the device, it does not define it)."""
    c = np.zeros(64, F32)
    c[:len(e)] = np.asarray(e, F32)
    v = c.copy()
    off = 1
    while off < 64:
        prev = c.copy()
        c[off:] = prev[off:] + prev[:-off]
        off *= 2
    lanes = np.arange(64)
    off = 32
    while off:
        v = (v + v[lanes ^ off]).astype(F32)
        off //= 2
    return c, v[0]


def follower_sample_case(A, via_a_num, special=None, seed=0):
    """Inputs of one sf_follower_glue_fwd launch with feedback 2: logits, validity, targets, flags as in
    follower_glue_case, and the launch's (sample seed, stream, row0).  Row kinds, by position:
      every a_num of 1 .. A; through is_valid also masks with holes: an invalid candidate between valid ones, candidate 0
      invalid, only the last candidate valid; rows moved by SHIFTS; rows whose valid candidates span more than UNDERFLOW
      (the head within a few units of the maximum, the tail below expf's float32 range); rows with one valid candidate.
    special 'zero' / 'one': row `at` of the launch is the global row whose uniform is exactly 0 / U_ONE (row0 is chosen
    for it; stream 1).  The 'zero' row has candidate 0 invalid (through is_valid) and a first valid candidate of solid
    weight; the 'one' row has every candidate valid, a head of ordinary weights and a tail that underflows in float32,
    drawn until f32_lane_sums predicts that a draw which looks at cdf > u * sum alone lands on the tail (case['zero_pick']):
    either no lane exceeds u * sum and the highest valid lane is taken, or a tail lane's sum, rounded in another order
    than the last head lane's, is the first to exceed it.  special 'half': the row's uniform is exactly 0.5 and its
    weights are 1 in candidates (A - 1) // 2 and A - 1 and 0 in float32 elsewhere, so that u * sum is a prefix sum and
    every float32 operation is exact: `cdf > u * sum` takes the second of the two, `>=` would take the first."""
    rng = np.random.default_rng([3000, A, seed, int(via_a_num), {None: 0, 'zero': 1, 'one': 2, 'half': 3}[special]])
    B = 4 * max(A, 32)                                          # (one row unclear by design still leaves 0.99 clear)
    x, sh = shifted_rows(rng, B, A)
    a_num = (1 + rng.permutation(B) % A).astype(np.int32)
    at = B // 2 + 1
    if special:
        a_num[at] = A
    valid = np.arange(A)[None, :] < a_num[:, None]
    hole = np.zeros(B, np.int64)                                # 0 prefix, 1 a hole inside, 2 candidate 0 invalid, 3 last only
    wide = np.zeros(B, bool)
    for i in range(B):
        n = int(a_num[i])
        x[i, n:] = x[i, :n].max() + F32(1 + 7 * rng.random())   # masked candidates score ABOVE every valid one
        if not via_a_num and i != at:
            k = (i // 2) % 4
            if k == 1 and n >= 3:
                hole[i] = 1
                valid[i, int(rng.integers(1, n - 1))] = False
            elif k == 2 and n >= 2:
                hole[i] = 2
                valid[i, 0] = False
            elif k == 3 and A >= 2:
                hole[i] = 3
                valid[i] = False
                valid[i, A - 1] = True
                x[i, A - 1] = x[i, 0]
        v = np.flatnonzero(valid[i])
        if i % 7 == 5 and len(v) >= 2 and i != at:              # a tail below float32's exp
            wide[i] = True
            tail = v[(len(v) + 1) // 2:] if i % 14 == 5 else v[:len(v) // 2]
            x[i, tail] = (x[i, np.setdiff1d(v, tail)].max() - (UNDERFLOW + 2 + 30 * rng.random(len(tail)))).astype(F32)
    stream, row0, zero_pick = seed, 1000, False
    if special:
        where = dict(zero=U_ZERO_AT, one=U_ONE_AT, half=U_HALF_AT)[special]
        stream, row0 = where['stream'], where['row'] - at
        sh[at] = 0.0
        x[at] = (rng.standard_normal(A) * 1.5).astype(F32)
        if special == 'zero' and not via_a_num and A >= 2:
            valid[at, 0] = False
        if special == 'half':                                   # two equal maxima, nothing else within float32's exp
            x[at] -= F32(2 * UNDERFLOW)
            x[at, [(A - 1) // 2, A - 1]] = F32(1.25)
            wide[at] = A > 2
        if special == 'one' and A >= 2:
            head = (A + 1) // 2
            for _ in range(400):
                x[at] = (rng.standard_normal(A) * 1.5).astype(F32)
                x[at, head:] = (x[at, :head].max() - (UNDERFLOW + 2 + 30 * rng.random(A - head))).astype(F32)
                e = np.exp((x[at] - x[at].max()).astype(F32)).astype(F32)
                cdf, se = f32_lane_sums(e)
                hit = np.flatnonzero(cdf[:A] > F32(F32(U_ONE) * se))
                zero_pick = e[hit[0] if len(hit) else A - 1] == 0
                if zero_pick:
                    break
            wide[at] = True
    target = np.zeros(B, np.int64)
    for i in range(B):
        v, nv = np.flatnonzero(valid[i]), np.flatnonzero(~valid[i])
        tk = int(rng.integers(0, 4))
        target[i] = int(rng.choice(nv)) if tk == 1 and len(nv) else (-1 if tk == 2 else int(rng.choice(v)))
    ended = (rng.random(B) < 0.25).astype(np.uint8)
    return dict(logit=x, shift=sh, a_num=a_num, valid=valid, target=target, ended=ended, hole=hole, wide=wide,
                seed=SAMPLE_SEED, stream=stream, row0=row0, at=at if special else None, zero_pick=bool(zero_pick))


# the launches of tests/test_gpu_choice_kernels.py, section 6: (A, via_a_num, special).  Every one keeps a clear share of
# at least 0.99 (tests/test_choice_models_host.py asserts it on the mirror alone).
SAMPLE_CASES = [(A, v, None) for A in (1, 2, 9, 16, 63, 64) for v in (False, True)] + \
               [(A, v, s) for A in (2, 9, 16, 64) for v in (False, True) for s in ('zero', 'one')] + \
               [(A, v, 'half') for A in (2, 16, 64) for v in (False, True)]


def sample_expectation(case):
    """The mirror's side of one case: dict(u, a, margin, lo, hi, clear) -- lo / hi the mirror's actions at u * (1 -+ CLEAR),
    the two an unclear row may take."""
    masked = np.where(case['valid'], case['logit'], F32(-np.inf)).astype(F32)
    B = len(masked)
    u = follower_uniforms(case['seed'], case['stream'], case['row0'], B)
    return draw_expectation(masked, case['valid'], u)


def draw_expectation(masked, valid, u):
    a, margin = follower_draws(masked, valid, u)
    lo = follower_draws(masked, valid, u, -CLEAR)[0]
    hi = follower_draws(masked, valid, u, +CLEAR)[0]
    return dict(u=u, a=a, margin=margin, lo=lo, hi=hi, clear=margin > CLEAR)


def check_draws(what, a, masked, valid, ex):
    """The draw-by-draw rule: a clear row takes the mirror's action, an unclear one the mirror's action at
    u * (1 - CLEAR) or u * (1 + CLEAR); every action is a valid candidate whose logit is finite and whose float32 weight
    exp(l - max) is not 0.  Returns the clear share."""
    rows = np.arange(len(a))
    assert ((a >= 0) & (a < masked.shape[1])).all(), what
    clear = ex['clear']
    l = masked[rows, a]
    assert valid[rows, a].all() and np.isfinite(l).all(), what
    top = np.where(valid, masked, F32(-np.inf)).max(1)
    bad = np.flatnonzero(top - l > UNDERFLOW)
    assert len(bad) == 0, '%s: row %d took candidate %d, %.1f below the maximum: its float32 probability is exactly 0' % (
        what, bad[0], a[bad[0]], (top - l)[bad[0]])
    bad = np.flatnonzero(clear & (a != ex['a']))
    assert len(bad) == 0, '%s: %d clear rows differ from the mirror, first %d: got %d, mirror %d (u %.9g, margin %.3g)' % (
        what, len(bad), bad[0], a[bad[0]], ex['a'][bad[0]], ex['u'][bad[0]], ex['margin'][bad[0]])
    bad = np.flatnonzero(~clear & (a != ex['lo']) & (a != ex['hi']))
    assert len(bad) == 0, '%s: unclear row %d took %d, the mirror allows %d or %d' % (
        what, bad[0] if len(bad) else -1, a[bad[0]] if len(bad) else -1, ex['lo'][bad[0]] if len(bad) else -1,
        ex['hi'][bad[0]] if len(bad) else -1)
    return float(clear.mean())


def check_sample_scores(what, got_score, masked, a, shift):
    """score = log p(action taken) by check_values, the rows of every shift on their own -> [(shift, e, e32)]."""
    rows = np.arange(len(a))
    r = masked.astype(np.float64)[rows, a] - lse(masked, np.float64)
    f = masked[rows, a] - lse(masked, F32)
    out = []
    for sh in sorted(set(shift.tolist())):
        sel = shift == sh
        out.append((sh,) + check_values('%s shift %g score' % (what, sh), got_score[sel], r[sel], f[sel]))
    return out


def chi2_rows():
    """The fixed logit rows of the chi-square tests: (name, row float32 [A], valid bool [A])."""
    out = []
    for A in (9, 64):
        for temp in (0.5, 2.5):
            row = (np.random.default_rng([5, A]).standard_normal(A) * temp).astype(F32)
            out.append(('A %d temp %g' % (A, temp), row, np.ones(A, bool)))
    row = (np.random.default_rng([5, 9, 1]).standard_normal(9) * 1.5).astype(F32)
    valid = np.ones(9, bool)
    valid[[0, 2, 3, 6, 8]] = False                                 # 5 of 9 masked, candidate 0 and the last among them
    row[~valid] += F32(6)                                          # (and they hold the largest numbers)
    out.append(('A 9, 5 masked', row, valid))
    return out


CHI2_N, CHI2_STREAM, CHI2_ROW0 = 40000, 3, 99
