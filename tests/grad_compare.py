"""Element-wise comparison of training gradients against a float64 reference (tests/test_gpu_grads_f64.py).

For a HIP gradient g, the float64 oracle's r and the fp32 oracle's f -- same inputs, same dropout masks -- of one
parameter:

    e   = max|g - r| / max|r|      the HIP path's distance to exact arithmetic
    e32 = max|f - r| / max|r|      the reference's own fp32 arithmetic's distance to it

and the bound is  e <= max(K * e32, FLOOR)  and  e <= CEILING.  The same bound holds per BLOCK relative to the block's
own maximum -- never tighter than the tensor's bound, which roundoff carried in from upstream (the gradient reaching every
row of a block) may use up -- and blocks whose reference maximum is below BLOCK_SMALL of the tensor's are held to the
tensor bound only:

    LSTM weights      4 gates x the column segments of the concatenated input (`lstm_blocks`)
    LSTM biases       4 gates
    text attention    the two halves of linear_out ([weighted context | h])
    embeddings        every row (`row_blocks`); a row whose reference is zero by construction -- the padding token, a
                      token absent from the batch -- must be EXACTLY zero

A parameter whose exact gradient is zero (a bias added to every candidate's score: the softmax is shift-invariant) has
no scale of its own: its HIP gradient is held to K x the fp32 reference's own roundoff of that zero (max|f|), and never
less than ZERO_REL x the largest gradient of the set.  Every tensor prints e and e32 (pytest -s), so drift is visible
long before it fails.  `norm_sample_check` is the older check (L2 norm + 16 sampled entries at rtol 3e-3) that
tests/test_grad_compare.py shows to accept corruptions this comparator rejects.
"""
import numpy as np

K = 4.0
FLOOR = 2e-6
CEILING = 1e-4
BLOCK_SMALL = 1e-3
ZERO_REL = 1e-7


def _np(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, np.float64)


def lstm_blocks(rows, col_edges=None, cols=None):
    """Blocks of an LSTM weight [4H, K] (gate order i, f, g, o): 4 gates x the column segments [(label, c0, c1)]
    (default: one segment of all `cols`); for a bias [4H] pass neither."""
    H = rows // 4
    gates = [(gname, slice(k * H, (k + 1) * H)) for k, gname in enumerate('ifgo')]
    if col_edges is None and cols is None:
        return [(gname, (rs,)) for gname, rs in gates]
    segs = col_edges if col_edges is not None else [('all', 0, cols)]
    return [('%s/%s' % (gname, lab), (rs, slice(c0, c1))) for gname, rs in gates for lab, c0, c1 in segs]


def halves_blocks(cols, rows):
    """linear_out of the text attention [H, 2H]: [weighted context | h] (model.py:141)."""
    h = cols // 2
    return [('weighted', (slice(0, rows), slice(0, h))), ('h', (slice(0, rows), slice(h, cols)))]


def row_blocks(n_rows):
    return [('row %d' % i, (i,)) for i in range(n_rows)]


class Report:
    def __init__(self):
        self.rows = []            # (name, e, e32, bound)

    def worst(self):
        """The tensor with the largest e: (name, e, e32)."""
        return max(self.rows, key=lambda r: r[1])[:3] if self.rows else None


def _rel(d, scale):
    return d / scale if scale > 0 else (0.0 if d == 0 else np.inf)


def compare_grads(hip, f64, f32, blocks=None, what='', k=K, floor=FLOOR, ceiling=CEILING, report=None):
    """hip / f64 / f32: {name: gradient}.  blocks: {name: [(label, index)]} (see the *_blocks helpers); a name whose
    blocks are `row_blocks` also gets the exact-zero rule for rows whose reference is zero.  Every name of f64 must be
    in hip and f32.  Returns a Report; raises AssertionError naming the first tensor / block that breaks the bound."""
    blocks = blocks or {}
    report = report if report is not None else Report()
    R = {n: _np(v) for n, v in f64.items()}
    largest = max(float(np.abs(r).max()) for r in R.values())
    errors = []
    for name, r in R.items():
        assert name in hip and hip[name] is not None, '%s %s: no HIP gradient' % (what, name)
        g, f = _np(hip[name]), _np(f32[name])
        assert g.shape == r.shape == f.shape, (what, name, g.shape, r.shape, f.shape)
        if not np.isfinite(g).all():
            errors.append('%s %s: non-finite HIP gradient' % (what, name))
            continue
        scale = float(np.abs(r).max())
        if scale <= 1e-9 * largest:                 # exact gradient zero (shift invariance)
            gm, fm = float(np.abs(g).max()), float(np.abs(f).max())
            zb = max(k * fm, ZERO_REL * largest)
            print('[grad] %s %-44s exact zero: max|g| = %.2e, fp32 reference %.2e (bound %.1e; largest gradient %.2e)'
                  % (what, name, gm, fm, zb, largest))
            if gm > zb:
                errors.append('%s %s: exact gradient is zero, max|g| = %.3e > max(K x fp32 reference %.3e, %.0e x largest %.3e)'
                              % (what, name, gm, fm, ZERO_REL, largest))
            continue
        e = _rel(float(np.abs(g - r).max()), scale)
        e32 = _rel(float(np.abs(f - r).max()), scale)
        bound = min(max(k * e32, floor), ceiling)
        report.rows.append((name, e, e32, bound))
        worst_blk = ''
        bad = []
        is_rows = False
        for label, idx in blocks.get(name, ()):
            is_rows = is_rows or label.startswith('row ')
            rb, gb, fb = r[idx], g[idx], f[idx]
            bs = float(np.abs(rb).max())
            if is_rows and bs == 0.0:
                if np.any(gb != 0.0):
                    bad.append('%s: reference zero by construction, max|g| = %.3e' % (label, float(np.abs(gb).max())))
                continue
            if bs < BLOCK_SMALL * scale:
                continue
            eb = _rel(float(np.abs(gb - rb).max()), bs)
            e32b = _rel(float(np.abs(fb - rb).max()), bs)
            bb = min(max(k * e32b, k * e32, floor), ceiling)
            if not worst_blk or eb / bb > worst_blk[0]:
                worst_blk = (eb / bb, '%s e=%.2e e32=%.2e' % (label, eb, e32b))
            if eb > bb:
                bad.append('%s: e = %.3e > %.3e (e32 = %.3e)' % (label, eb, bb, e32b))
        print('[grad] %s %-44s e = %.2e  e32 = %.2e  (bound %.1e)%s' % (
            what, name, e, e32, bound, ('  worst block ' + worst_blk[1]) if worst_blk else ''))
        if e > bound:
            errors.append('%s %s: e = %.3e > bound %.3e (e32 = %.3e, K = %g, floor %.0e, ceiling %.0e)'
                          % (what, name, e, bound, e32, k, floor, ceiling))
        if bad:
            errors.append('%s %s: %d block(s) out of bound, first: %s' % (what, name, len(bad), bad[0]))
    assert not errors, '\n'.join(errors)
    return report


def norm_sample_check(hip, ref, rng, n_samples=16, rtol=3e-3):
    """The older end-to-end check (tests/golden/make_golden.py grads_summary + tests/test_gpu_follower.py::_check_grads):
    per parameter the L2 norm and `n_samples` randomly drawn entries, at rtol 3e-3.  Raises AssertionError."""
    gmax = max(float(np.sqrt(np.sum(_np(v) ** 2))) for v in ref.values())
    for name, rv in ref.items():
        r = _np(rv).ravel()
        flat = _np(hip[name]).ravel()
        rn = float(np.sqrt(np.sum(r ** 2)))
        norm = float(np.sqrt(np.sum(flat ** 2)))
        if rn < 1e-6 * max(gmax, 1.0):
            assert norm < 1e-5 * max(gmax, 1.0), name
            continue
        idx = rng.integers(0, r.size, size=min(n_samples, r.size))
        np.testing.assert_allclose(norm, rn, rtol=rtol, err_msg=name)
        np.testing.assert_allclose(flat[idx], r[idx], rtol=rtol, atol=rtol * rn / np.sqrt(r.size) + 1e-7, err_msg=name)
