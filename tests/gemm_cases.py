"""Inputs and shapes for tests/test_gpu_gemm_dispatch.py (checked on the host by tests/test_gemm_cases_host.py).

Two families of operands make a product EXACT in float32 whatever kernel forms it, however it splits the reduction and
in whatever order it adds:

  * selection ('selw' / 'selx' forward, 'sely' / 'selx' backward): one operand is random float32 with all 24 mantissa
    bits in use and magnitudes in [0.5, 2); the other has exactly one non-zero, +-2^e with e in [-3, 3], per output
    column (or row) of the reduction, at position (a * i + b) mod K with a coprime to K.  Every output element is one
    operand element times a power of two; every other product is a true zero.  Through the error-free three-way bf16
    split the three pieces of the dense operand (8 + 8 + 8 mantissa bits) re-add exactly in any order.
  * small integers ('int'): every operand, bias and initial value of an accumulated output is an integer in [-8, 8]
    stored as float32, so every partial sum is an integer of magnitude <= 64 * max(K, M) + 8 < 2^24: exact.

`layout` pads an operand into a wider buffer the way the engines hand views into wider rows to the library: NaN in the
padding columns and in two rows behind the last one for inputs, a sentinel for outputs.

The case tables name, per shape, the kernel(s) of csrc/sf_gemm.hip the dispatch must launch for it (spelled as
`_lib.kernel_profile()` reports them).  They are the smallest shapes that reach each branch.  The names are checked
twice: on the GPU against the profile of the launches, and on the host by tests/test_gemm_plan_host.py, which asks the
dispatch's plan functions (csrc/sf_gemm_plan.h, pure host code) for the kernels of every row."""
import math
from collections import namedtuple

import numpy as np

SENTINEL = np.float32(-1234.5)          # what the padding of an output holds before and must hold after a call
TAIL_ROWS = 2                           # poisoned rows behind the last row of every operand
INT_LIMIT = 2 ** 24


# ---------------------------------------------------------------------------------------- operands
def full_mantissa(rng, *shape):
    """float32 in +-[0.5, 2) whose 24 mantissa bits are all in play (the lowest one is set in half of the elements)."""
    m = rng.integers(2 ** 23, 2 ** 24, shape).astype(np.float64) * 2.0 ** -24          # [0.5, 1), 24 bits
    v = m * rng.choice([1.0, 2.0], shape) * rng.choice([-1.0, 1.0], shape)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def small_ints(rng, *shape):
    return rng.integers(-8, 9, shape).astype(np.float32)


def coprime_step(K, start=7):
    a = start
    while math.gcd(a, K) != 1:
        a += 1
    return a


def selection(rng, rows, K):
    """[rows, K] with one non-zero +-2^e (e in [-3, 3]) per row, at column (a * r + b) mod K, a coprime to K: the
    columns differ from row to row (no symmetry to hide a swapped fragment) and cover all of K when rows >= K.
    Returns (matrix, column of each row, value of each row)."""
    a, b = coprime_step(K), 3
    col = (a * np.arange(rows, dtype=np.int64) + b) % K
    val = (rng.choice([-1.0, 1.0], rows) * 2.0 ** rng.integers(-3, 4, rows)).astype(np.float32)
    m = np.zeros((rows, K), np.float32)
    m[np.arange(rows), col] = val
    return m, col, val


def int_matmul(a, b):
    """a @ b of integer-valued arrays as int64.  Small products run numpy's int64 matmul itself; the large ones run
    the float64 BLAS product, which is the same integer exactly (every partial sum is far below 2^53) and takes
    milliseconds where the int64 loop takes many seconds."""
    ai, bi = np.rint(a).astype(np.int64), np.rint(b).astype(np.int64)
    assert np.array_equal(ai, a) and np.array_equal(bi, b)
    if a.shape[0] * a.shape[1] * b.shape[1] <= 1 << 26:
        return ai @ bi
    assert float(np.abs(ai).max()) * float(np.abs(bi).max()) * a.shape[1] < 2.0 ** 52
    return np.rint(a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


def as_f32_exact(v):
    """An exact reference (int64 or float64) as float32, asserting that nothing is lost on the way."""
    out = np.asarray(v).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), np.asarray(v).astype(np.float64)), 'reference is not exact in float32'
    return out


FwdInputs = namedtuple('FwdInputs', 'x w b ref')            # ref: float32 [M, N], exact
BwdInputs = namedtuple('BwdInputs', 'x w dy dx0 dw0 db0 dx dw db')   # dx/dw/db: exact float32 results (dx None: not asked)

FWD_FAMILIES = ('int', 'selw', 'selx')
BWD_FAMILIES = ('int', 'sely', 'selx')


def forward_inputs(family, M, N, Ks, seed=0):
    """Operands of y = sum_s x_s w_s^T (+ b) for the reduction segments Ks (one or two) and the exact result.
    x and w are lists with one array per segment.  The selection families have no bias (the sum would round)."""
    rng = np.random.default_rng([seed, M, N, sum(Ks), FWD_FAMILIES.index(family)])
    xs, ws = [], []
    if family == 'int':
        assert 64 * max(sum(Ks), M) + 8 < INT_LIMIT
        for K in Ks:
            xs.append(small_ints(rng, M, K))
            ws.append(small_ints(rng, N, K))
        b = small_ints(rng, N)
        ref = sum(int_matmul(x, w.T) for x, w in zip(xs, ws)) + np.rint(b).astype(np.int64)
        return FwdInputs(xs, ws, b, as_f32_exact(ref))
    # selection: the one non-zero of an output column (selw) / row (selx) lies in ONE of the segments
    Kt = sum(Ks)
    if family == 'selw':
        dense, (sel, col, val) = full_mantissa(rng, M, Kt), selection(rng, N, Kt)
        ref = dense[:, col] * val[None, :]
        xcat, wcat = dense, sel
    else:
        dense, (sel, col, val) = full_mantissa(rng, N, Kt), selection(rng, M, Kt)
        ref = (dense[:, col] * val[None, :]).T
        xcat, wcat = sel, dense
    k0 = 0
    for K in Ks:
        xs.append(np.ascontiguousarray(xcat[:, k0:k0 + K]))
        ws.append(np.ascontiguousarray(wcat[:, k0:k0 + K]))
        k0 += K
    return FwdInputs(xs, ws, None, as_f32_exact(ref.astype(np.float64)))


def backward_inputs(family, M, N, K, accumulate_dx, seed=0):
    """Operands of sf_linear_bwd with act = 0 (dx = dy w, dw += dy^T x, db += colsum dy) and the exact results.
      int : everything small integers.
      sely: dy has one +-2^e per column n (at row (a n + b) mod M), x is full-mantissa, w small integers:
            dw[n, :] = +-2^e x[m(n), :], db[n] = +-2^e, dx = sums of a few small integers times powers of two.
      selx: x has one +-2^e per column k (at row (a k + b) mod M), dy is full-mantissa: dw[n, k] = +-2^e dy[m(k), n];
            dx and db are dense float sums here and are not asked for (None).
    dw and db start from non-zero integers; in the selection families the reference adds them in ONE float32 rounding
    (the product itself is exact, so a kernel that forms it and then adds the old value rounds once, like the reference)."""
    rng = np.random.default_rng([seed, M, N, K, BWD_FAMILIES.index(family), accumulate_dx])
    dx0 = small_ints(rng, M, K)
    dw0 = small_ints(rng, N, K)
    dw0[dw0 == 0] = 3.0
    db0 = small_ints(rng, N)
    db0[db0 == 0] = -5.0
    f64 = np.float64
    if family == 'int':
        assert 64 * max(K, M, N) + 8 < INT_LIMIT
        x, w, dy = small_ints(rng, M, K), small_ints(rng, N, K), small_ints(rng, M, N)
        dx = int_matmul(dy, w) + (np.rint(dx0).astype(np.int64) if accumulate_dx else 0)
        dw = int_matmul(dy.T, x) + np.rint(dw0).astype(np.int64)
        db = np.rint(dy).astype(np.int64).sum(0) + np.rint(db0).astype(np.int64)
        return BwdInputs(x, w, dy, dx0, dw0, db0, as_f32_exact(dx), as_f32_exact(dw), as_f32_exact(db))
    if family == 'sely':
        selT, row, val = selection(rng, N, M)               # [N, M]: column n of dy has its non-zero at row[n]
        dy = np.ascontiguousarray(selT.T)
        x, w = full_mantissa(rng, M, K), small_ints(rng, N, K)
        dx = as_f32_exact(dy.astype(f64) @ w.astype(f64) + (dx0.astype(f64) if accumulate_dx else 0.0))
        dw = (dw0.astype(f64) + (x[row, :] * val[:, None]).astype(f64)).astype(np.float32)       # one rounding
        db = as_f32_exact(db0.astype(f64) + val.astype(f64))
        return BwdInputs(x, w, dy, dx0, dw0, db0, dx, dw, db)
    selT, row, val = selection(rng, K, M)                   # [K, M]: column k of x has its non-zero at row[k]
    x = np.ascontiguousarray(selT.T)
    dy, w = full_mantissa(rng, M, N), small_ints(rng, N, K)
    dw = (dw0.astype(f64) + (dy[row, :] * val[:, None]).T.astype(f64)).astype(np.float32)
    return BwdInputs(x, w, dy, dx0, dw0, db0, None, dw, None)


# ------------------------------------------------------------------------------------------ layouts
def layout(a, ld=None, fill=np.nan):
    """`a` ([rows, cols] or [n]) inside a buffer [rows + TAIL_ROWS, ld] (or [n + TAIL_ROWS]) filled with `fill`: the
    padding columns cols..ld-1 of every row and the rows behind the last one are not the operand's."""
    a = np.asarray(a, np.float32)
    if a.ndim == 1:
        buf = np.full(a.shape[0] + TAIL_ROWS, fill, np.float32)
        buf[:a.shape[0]] = a
        return buf
    rows, cols = a.shape
    ld = cols if ld is None else ld
    assert ld >= cols
    buf = np.full((rows + TAIL_ROWS, ld), fill, np.float32)
    buf[:rows, :cols] = a
    return buf


def outside_is_untouched(buf, rows, cols, fill=SENTINEL):
    """Whether everything of a `layout` buffer outside [rows, cols] still holds `fill`, bit for bit."""
    bits = np.asarray(buf, np.float32).view(np.uint32)
    want = np.float32(fill).view(np.uint32)
    if bits.ndim == 1:
        return bool((bits[rows:] == want).all())
    return bool((bits[:rows, cols:] == want).all() and (bits[rows:] == want).all())


def pads(strided, index):
    """(j_a, j_b) of the row strides `width + 4 * j` of a case's two strided operands: (0, 0) contiguous, else (1, 3)
    or (3, 1) by the case's position in its table, so that both paddings meet every kernel family."""
    if not strided:
        return 0, 0
    return (1, 3) if index % 2 == 0 else (3, 1)


# -------------------------------------------------------------------------------------------- cases
SMALL = 'gemm_nt_small_kernel<%d, %d>'
NT, SPLIT, TILED, BIG = 'gemm_nt_kernel<%d>', 'gemm_nt_split_kernel<%d>', 'gemm_nt_tiled_kernel<%d>', 'gemm_nt_big_kernel'
NN, TN, TN_TILED, TN_SPLIT = 'gemm_nn_kernel<%d>', 'gemm_tn_kernel', 'gemm_tn_tiled_kernel', 'gemm_tn_split_kernel'
REDUCE, COLSUM, COLSUM_FINISH, TRANSPOSE = 'reduce_slabs_kernel', 'colsum_kernel', 'colsum_finish_kernel', 'transpose_kernel'

# forward through sf_linear_fwd: kernels that must be launched, kernels that must NOT, M, N, K, and whether the case runs
# under sf_debug_gate_product_f32(1)
Fwd = namedtuple('Fwd', 'kernels absent M N K f32')


def _fwd(kernels, M, N, K, absent=(), f32=0):
    kernels = (kernels,) if isinstance(kernels, str) else tuple(kernels)
    return Fwd(kernels, tuple(absent), M, N, K, f32)


def _forward_cases():
    c = []
    # the short-reduction kernel, all ten instantiations; then M at the ragged edge of the tile count and N = 2044
    c += [_fwd(SMALL % (1, 2), 1, 16, 4), _fwd(SMALL % (1, 2), 48, 80, 32),
          _fwd(SMALL % (1, 4), 1, 16, 300), _fwd(SMALL % (1, 4), 7, 2048, 300),
          _fwd(SMALL % (1, 8), 1, 16, 1024), _fwd(SMALL % (1, 16), 1, 16, 1028), _fwd(SMALL % (1, 18), 1, 16, 2176)]
    for M in (33, 47):
        c += [_fwd(SMALL % (2, 2), M, N, 4) for N in (2048, 2044)]
        c += [_fwd(SMALL % (2, 4), M, N, 300) for N in (2048, 2044)]
        c += [_fwd(SMALL % (2, 8), M, N, 1024) for N in (2048, 2044)]
    for M in (65, 79):
        c += [_fwd(SMALL % (4, 2), M, N, 4) for N in (2048, 2044)]
        c += [_fwd(SMALL % (4, 4), M, N, 300) for N in (2048, 2044)]
    c += [_fwd(SMALL % (1, 2), 1, 2044, 4), _fwd(SMALL % (1, 8), 15, 2044, 1024), _fwd(SMALL % (1, 16), 1, 20, 1028),
          _fwd(SMALL % (1, 18), 15, 20, 2176)]
    # the streaming kernel: one block of rows, 8 K splits + the slab reduction; a partial last chunk; a ragged column tile
    for i, M in enumerate((1, 17, 33, 49, 65, 81, 97, 113)):
        for N, K in ((16, 2368), (16, 2372), (20, 2372)):
            c.append(_fwd((NT % (i + 1), REDUCE), M, N, K))
    c += [_fwd((NT % 8, REDUCE), M, 16, 2368) for M in (129, 300, 513)]           # 2, 3 and 5 row blocks
    c.append(_fwd(NT % 1, 300, 2048, 4, absent=(REDUCE,)))                        # 19 row blocks, the fused epilogue
    # the gate product's kernels on the bf16 matrix cores, and the fp32 LDS-tiled kernel they replace
    for M in (1, 16, 17, 32, 33, 49, 65, 80, 81, 97, 113, 128):
        mt = (M + 15) // 16
        for N in (64, 128):
            c.append(_fwd((SPLIT % mt, REDUCE), M, N, 2368))
            c.append(_fwd((TILED % mt, REDUCE), M, N, 2368, f32=1))
    # the many-row kernel: ragged tiles, a partial last stage, and each of its thresholds (M >= 512, N >= 64, four
    # chunks of K).  The short-reduction kernel comes first in the dispatch and takes every output of up to 2 048
    # 16 x 16 tiles while K <= 2 304, (515, 130, 96) and (512, 64, 32) among them: hence K = 2 320 at the narrow shapes.
    c += [_fwd(BIG, 513, 1024, 64), _fwd(BIG, 515, 130, 2324), _fwd(BIG, 512, 64, 2320), _fwd(BIG, 512, 1040, 52)]
    c.append(_fwd((NT % 8, REDUCE), 511, 64, 2320, absent=(BIG,)))                # one row short: goes elsewhere
    c += [_fwd(SMALL % (1, 2), 515, 130, 96, absent=(BIG,)), _fwd(SMALL % (1, 2), 512, 64, 32, absent=(BIG,)),
          _fwd(SMALL % (1, 2), 511, 64, 32, absent=(BIG,))]
    return c


FORWARD = _forward_cases()

# two segments through sf_linear_slabs_fwd (raw slabs in the workspace): kernel, M, N, K1, K2
Slabs = namedtuple('Slabs', 'kernels M N K1 K2')
SLABS = ([Slabs((SPLIT % mt,), M, 64, 2368, 512) for mt, M in ((2, 17), (5, 65), (6, 81))] +     # boundary inside a K split
         [Slabs((NT % mt,), M, 64, 1028, 1344) for mt, M in ((2, 17), (5, 65), (6, 81))])        # partial chunk mid-reduction

# backward through sf_linear_bwd: kernels (name -> number of launches, 0 = must not run), M, N, K, accumulate_dx,
# whether dx is asked for, and the value of sf_debug_tn_split_min_rows (-1: the default)
Bwd = namedtuple('Bwd', 'kernels M N K accumulate_dx with_dx tn_split_min_rows')


def _bwd(kernels, M, N, K, accumulate_dx=0, with_dx=True, rows=-1):
    return Bwd(tuple(sorted(kernels.items())), M, N, K, accumulate_dx, with_dx, rows)


def _backward_cases():
    c = []
    # dx: gemm_nn_kernel<1|2|4|7>, unsplit (N = 16) and as 4 slabs (N = 256), one and two row blocks, dx overwritten and added to
    for M in (1, 16, 17, 32, 33, 64, 65, 112, 113):
        mtiles = (M + 15) // 16
        mt = 1 if mtiles <= 1 else 2 if mtiles <= 2 else 4 if mtiles <= 4 else 7
        for acc in (0, 1):
            c.append(_bwd({NN % mt: 1, TN: 1, COLSUM: 1, REDUCE: 0, COLSUM_FINISH: 0}, M, 16, 64, acc))
            c.append(_bwd({NN % mt: 1, TN: 1, COLSUM: 1, REDUCE: 1}, M, 256, 64, acc))
    # dW: gemm_tn_kernel unsplit, as row slabs, and with the column cut (main columns unsplit + a row-split tail)
    c.append(_bwd({TN: 1, REDUCE: 0}, 33, 64, 64))
    c.append(_bwd({TN: 1, REDUCE: 1, COLSUM: 1, COLSUM_FINISH: 1}, 128, 64, 16))
    c.append(_bwd({TN: 1}, 250, 2048, 300))
    c.append(_bwd({TN: 2, REDUCE: 1}, 512, 2048, 4352, with_dx=False))
    c.append(_bwd({TN_TILED: 1, TN: 0}, 4097, 128, 132))
    c.append(_bwd({TN_SPLIT: 1, TN: 0}, 4096, 128, 128))
    c.append(_bwd({TN_SPLIT: 1, TN: 0}, 257, 384, 256, rows=256))
    c.append(_bwd({TRANSPOSE: 2, BIG: 1, TN: 0}, 1024, 64, 64))                   # the many-row form
    c.append(_bwd({TRANSPOSE: 2, BIG: 1, TN: 0}, 1028, 100, 300))
    return c


BACKWARD = _backward_cases()

# every instantiation the tables must name (tests/test_gemm_cases_host.py compares with a literal set of its own)
def named_kernels():
    names = set()
    for case in FORWARD:
        names.update(case.kernels)
    for case in SLABS:
        names.update(case.kernels)
    for case in BACKWARD:
        names.update(k for k, n in case.kernels if n > 0)
    return names


# ------------------------------------------------------------------------------ float64 family
# one dense-random shape per kernel family: (family name, kernel that must run, entry, M, N, K, f32 switch, tn rows)
Dense = namedtuple('Dense', 'family kernel entry M N K f32 tn_split_min_rows')
DENSE = [
    Dense('nt_small', SMALL % (2, 4), 'fwd', 47, 2044, 300, 0, -1),
    Dense('nt_stream', NT % 3, 'fwd', 37, 20, 2372, 0, -1),
    Dense('nt_split', SPLIT % 5, 'fwd', 70, 128, 2368, 0, -1),
    Dense('nt_tiled', TILED % 5, 'fwd', 70, 128, 2368, 1, -1),
    Dense('nt_big', BIG, 'fwd', 515, 130, 2324, 0, -1),
    Dense('nn', NN % 7, 'bwd', 113, 256, 64, 0, -1),
    Dense('tn', TN, 'bwd', 250, 2048, 300, 0, -1),
    Dense('tn_tiled', TN_TILED, 'bwd', 4097, 128, 132, 0, -1),
    Dense('tn_split', TN_SPLIT, 'bwd', 257, 384, 256, 0, 256),
    Dense('tn_many_row', BIG, 'bwd', 1028, 100, 300, 0, -1),
]


def dense_forward(M, N, K, seed=0):
    """The badly scaled, asymmetric operands of test_gpu_ops.py::test_many_row_product_on_the_bf16_matrix_cores."""
    rng = np.random.default_rng([seed, M, N, K])
    rnd = lambda *s: rng.standard_normal(s).astype(np.float32)
    x = (rnd(M, K) * (1.0 + 3.0 * (np.arange(K) % 7 == 0))[None, :] + 0.25).astype(np.float32)
    w = (rnd(N, K) * K ** -0.5 * (1.0 + (np.arange(N) % 5)[:, None])).astype(np.float32)
    return x, w, rnd(N)


def dense_backward(M, N, K, seed=0):
    """The operands of test_gpu_ops.py::test_weight_gradient_on_the_bf16_matrix_cores, plus initial dx and db."""
    rng = np.random.default_rng([seed, M, N, K, 1])
    rnd = lambda *s: rng.standard_normal(s).astype(np.float32)
    x = (rnd(M, K) + (np.arange(K) % 7)[None, :] * 0.1).astype(np.float32)
    dy = (rnd(M, N) * (1.0 + (np.arange(N) % 5)[None, :])).astype(np.float32)
    w = (rnd(N, K) * K ** -0.5).astype(np.float32)
    return x, w, dy, rnd(M, K), rnd(N, K), rnd(N)
