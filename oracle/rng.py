"""Oracle (test infrastructure): numpy mirror of the counter-based dropout mask the
HIP kernels generate (speaker_follower_amd/csrc/sf_common.h: sf_dropout_keep).

The reference uses torch's stateful nn.Dropout (model.py:52, 370, 414, 473); its
random stream cannot be reproduced, so train-mode parity is checked by giving the
oracle the *same* mask the device derives from (seed, stream, row, col).
"""
import numpy as np

_M = np.uint64(0xFFFFFFFF)


def _fmix32(h):
    h = h & _M
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M
    h ^= h >> np.uint64(16)
    return h


def dropout_bits(seed, stream, rows, cols):
    """uint32 hash for every (row, col) pair: rows [R] (global row ids), cols [C]."""
    rows = np.asarray(rows, np.uint64)[:, None]
    cols = np.asarray(cols, np.uint64)[None, :]
    key = _fmix32(np.uint64(seed) + np.uint64(0x9E3779B9) * np.uint64(stream))
    key = _fmix32(key ^ ((rows * np.uint64(0x85EBCA6B)) & _M))
    return _fmix32(key + ((cols * np.uint64(0x9E3779B9)) & _M)).astype(np.uint32)


def dropout_mask(seed, stream, rows, n_cols, p):
    """Multiplicative mask [R, n_cols] fp32: 0 with probability p, else 1/(1-p)."""
    if p <= 0.0:
        return np.ones((len(rows), n_cols), np.float32)
    thresh = np.uint32(min(int(p * 4294967296.0), 0xFFFFFFFF))
    bits = dropout_bits(seed, stream, rows, np.arange(n_cols))
    keep = bits >= thresh
    return keep.astype(np.float32) * np.float32(1.0 / (1.0 - p))


def sample_uniforms(seed, stream, rows):
    """(u1 [R], u2 [R]): the two uniforms of sf_sampling.h for global rows `rows` at (seed, stream)."""
    bits = dropout_bits(seed, stream, rows, [0, 1])
    return (bits[:, 0] >> np.uint32(8)).astype(np.float64) / 16777216.0, \
           (bits[:, 1] >> np.uint32(8)).astype(np.float64) / 16777216.0


def follower_sample(masked_row, valid_row, u):
    """float64 mirror of the follower's one-level inverse-CDF draw (speaker_follower_amd/csrc/sf_glue.h, feedback 2; the
    reference's Categorical sample at follower.py:491-497 draws from torch's stateful generator).  masked_row [A] logits
    (whatever stands on an invalid candidate is ignored), valid_row [A] bool with at least one finite valid logit, u the
    row's uniform: sample_uniforms(seed, sample_stream + site word, [row0 + b])[0].  e = exp(l - max) over the valid
    candidates and 0 elsewhere, cdf its inclusive sum in candidate order: the first valid candidate with cdf > u * sum,
    the highest valid candidate if there is none.  Returns (action, margin): margin = the smallest |cdf_i - u * sum| / sum
    over the valid candidates -- the device forms the same sums in fp32 (64 lanes, a 6-level shuffle scan), so a draw
    whose margin is ~1e-6 can fall on either side there."""
    l = np.asarray(masked_row, np.float64)
    valid = np.asarray(valid_row, bool)
    assert valid.any()
    e = np.zeros(len(l))
    e[valid] = np.exp(l[valid] - l[valid].max())
    cdf = np.cumsum(e)
    thr = u * cdf[-1]
    hit = np.flatnonzero(valid & (cdf > thr))
    a = int(hit[0]) if len(hit) else int(np.flatnonzero(valid)[-1])
    return a, float(np.min(np.abs(cdf[valid] - thr)) / cdf[-1])


def speaker_sample(logit_row, u1, u2, slot=32, underflow=None, detail=False):
    """float64 mirror of the device's two-level inverse-CDF draw (speaker_follower_amd/csrc/sf_sampling.h; the
    reference's D.Categorical(probs).sample() at speaker.py:170-174 draws from torch's stateful generator, which cannot be
    reproduced).  Returns (word, margin): margin = the smallest relative distance of either threshold to a CDF boundary
    of an item that carries weight -- fp32 roundoff on the device can flip a draw whose margin is ~1e-6.  (The margin
    differs from what it was before only where zero-weight items LEAD a prefix: their boundary at 0 no longer makes a draw at
    u ~ 0 look unclear; behind an item that carries weight a zero-weight item repeats that item's boundary.)

    The contract's edges, as sf_sampling.h states them: a slot with no finite column has weight 0 and is never chosen
    (its columns weigh 0 too, nothing here is NaN); a row with no finite column at all stays outside the contract
    (AssertionError); level 1 falls back to the slot of the arg max, level 2 to the LAST column of the slot WHOSE WEIGHT
    IS POSITIVE.  `underflow` (tests pass 104.0, where float32's expf reaches 0): a column more than that below its
    slot's maximum, and a slot whose maximum lies more than that below the row's, weigh exactly 0 as they do on the
    device, so "positive weight" means the same on both sides; None keeps every float64 weight.  detail=True returns
    (word, margin, info) with info = dict(slot, col, fallback1, fallback2, margin1, margin2, p = the slot weights, e =
    the column weights of the chosen slot)."""
    l = np.asarray(logit_row, np.float64)
    V = len(l)
    ns = (V + slot - 1) // slot
    seg = np.full(ns * slot, -np.inf)
    seg[:V] = l
    seg = seg.reshape(ns, slot)
    m_s = seg.max(1)
    live = m_s > -np.inf
    assert live.any(), 'a row without a finite column is outside the contract of the draw'
    d = seg - np.where(live, m_s, 0.0)[:, None]                        # (an empty slot: -inf throughout, weight 0)
    e_all = np.exp(d)
    M = m_s.max()
    ds = np.where(live, m_s - M, -np.inf)
    w = np.exp(ds)
    if underflow is not None:
        e_all[d < -underflow] = 0.0
        w[ds < -underflow] = 0.0
    z_s = e_all.sum(1)
    p = z_s * w
    cdf = np.cumsum(p)
    thr = u1 * cdf[-1]
    pos = p > 0
    hit = np.flatnonzero((cdf > thr) & pos)
    s = int(hit[0]) if len(hit) else int(np.argmax(l)) // slot
    margin1 = float(np.min(np.abs(cdf[pos] - thr)) / cdf[-1])
    e = e_all[s]
    c2 = np.cumsum(e)
    thr2 = u2 * z_s[s]
    pos2 = e > 0
    hit2 = np.flatnonzero((c2 > thr2) & pos2)
    c = int(hit2[0]) if len(hit2) else int(np.flatnonzero(pos2)[-1])
    margin2 = float(np.min(np.abs(c2[pos2] - thr2)) / z_s[s])
    word, margin = slot * s + c, min(margin1, margin2)
    if not detail:
        return word, margin
    return word, margin, dict(slot=s, col=c, fallback1=len(hit) == 0, fallback2=len(hit2) == 0, margin1=margin1,
                              margin2=margin2, p=p, e=e)
