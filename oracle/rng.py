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


def speaker_sample(logit_row, u1, u2, slot=32):
    """float64 mirror of the device's two-level inverse-CDF draw (speaker_follower_amd/csrc/sf_sampling.h; the
    reference's D.Categorical(probs).sample() at speaker.py:170-174 draws from torch's stateful generator, which cannot be
    reproduced).  Returns (word, margin): margin = the smallest relative distance of either threshold to a CDF boundary
    -- fp32 roundoff on the device can flip a draw whose margin is ~1e-6, so callers skip those."""
    l = np.asarray(logit_row, np.float64)
    V = len(l)
    ns = (V + slot - 1) // slot
    m_s = np.full(ns, -np.inf)
    z_s = np.zeros(ns)
    for s in range(ns):
        seg = l[slot * s:slot * (s + 1)]
        m_s[s] = seg.max()
        z_s[s] = np.exp(seg - m_s[s]).sum()
    M = m_s.max()
    p = z_s * np.exp(m_s - M)
    cdf = np.cumsum(p)
    thr = u1 * cdf[-1]
    hit = np.flatnonzero((cdf > thr) & (p > 0))
    s = int(hit[0]) if len(hit) else int(np.argmax(l)) // slot
    margin = np.min(np.abs(cdf - thr)) / cdf[-1]
    seg = l[slot * s:slot * (s + 1)]
    e = np.exp(seg - m_s[s])
    c2 = np.cumsum(e)
    thr2 = u2 * z_s[s]
    hit2 = np.flatnonzero((c2 > thr2) & (e > 0))
    c = int(hit2[0]) if len(hit2) else len(seg) - 1
    margin = min(margin, np.min(np.abs(c2 - thr2)) / z_s[s])
    return slot * s + c, float(margin)
