"""Case tables and plain numpy models of the kernels of csrc/sf_pointwise.hip that move data or step parameters: the
feature-table gathers (with the row loaders of csrc/sf_rows.h), the row movers of the searches, transpose / embedding /
fill / add / dropout, the small-parameter reducers of the scoring backward, and the fused Adam step.  The models follow
the contract in include/sf_hip.h and oracle/np_env.py (panorama_feature, action_embedding), not the kernels; no torch is
needed for them.  tests/test_mover_cases_host.py proves them on the CPU, tests/test_gpu_movers.py holds the kernels to
them on the GPU.

Everything but Adam is a copy, a select or a sum of small integers: compared bit for bit (`same_bits`).  Inputs are built
so that a wrong source shows as a wrong VALUE: every table element is a distinct binary16 number (so an fp32 and a
binary16 registration of the table must give the same bits), the sin/cos constants are four distinct numbers per
(row, candidate), every mover source counts its elements, and every destination starts as POISON, which must survive
wherever the contract names nothing.

One grid pass of the grid-stride kernels is GRID_PASS = 4096 blocks x 256 threads = 1 048 576 items; the case tables
hold one case above it per kernel (`big`), with tiny tables and only the row count large.
"""
from collections import namedtuple
from itertools import product

import numpy as np

F32 = np.float32
POISON = 0x7FC5BEEF                                               # a NaN pattern no kernel produces (int32 view)
GRID_PASS = 4096 * 256
ROW_MOVES_MAX = 4                                                  # include/sf_hip.h: SF_ROW_MOVES_MAX
N_VP = 3                                                           # viewpoints of every test table


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def poison(*shape):
    return np.full(shape, POISON, np.int32).view(F32)


def is_poison(a):
    return bits(a) == POISON


def same_bits(got, want, what=''):
    """Bit-for-bit equality (NaN poison and the sign of zero included); raises naming the first difference."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, '%s: %d of %d elements differ, first at %s: got %r, want %r' % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return True


# ================================================================================================ feature gathers
GatherCase = namedtuple('GatherCase', 'V IMG LOC A B')
GATHER_CASES = [GatherCase(*c) for c in (
    (1, 4, 16, 1, 1), (1, 8, 32, 2, 5), (1, 64, 128, 16, 67), (1, 4, 32, 16, 5),
    (3, 4, 16, 2, 1), (3, 8, 16, 1, 67), (3, 64, 32, 16, 5), (3, 8, 128, 2, 67), (3, 4, 128, 1, 5),
    (3, 64, 16, 16, 1), (3, 4, 32, 2, 67), (3, 8, 32, 16, 1),
    (36, 4, 16, 16, 5), (36, 8, 32, 1, 1), (36, 64, 128, 2, 5), (36, 64, 16, 2, 67), (36, 4, 128, 16, 1),
    (36, 8, 16, 2, 5), (36, 64, 32, 1, 67), (36, 4, 32, 1, 5), (36, 8, 128, 16, 67), (36, 64, 128, 1, 1),
    (1, 8, 16, 2, 67), (3, 64, 128, 2, 5),
)]
# B * V * (IMG + LOC) / 4 = 1 050 000 > GRID_PASS for the panorama, and B * (IMG + LOC) / 4 for the single-row entries
GATHER_BIG = GatherCase(1, 4, 16, 2, 210000)
LD_OUT = ('F', 'F+4', '2F')
ACT_EDGES = ('-1', '0', '1', 'a_num-1', 'a_num', 'A', 'A+3')
# refused shapes (include/sf_hip.h): nothing is launched, the output keeps its poison
REFUSED_CAND_SHAPES = [(8, 4), (8, 8), (8, 24), (6, 16)]            # (IMG, LOC): LOC % 16 or IMG % 4
REFUSED_PANO_SHAPES = [(6, 16), (6, 4)]                             # IMG % 4 (LOC 4, 8, 24 are panorama shapes)


def ld_out(kind, F):
    return {'F': F, 'F+4': F + 4, '2F': 2 * F}[kind]


def feature_table16(V, IMG, n_vp=N_VP):
    """[n_vp, V, IMG] binary16, every element a distinct finite normal number (consecutive bit patterns from the smallest
    normal up, odd elements negative)."""
    n = n_vp * V * IMG
    assert 0x0400 + n < 0x7C00
    k = np.arange(n, dtype=np.uint16)
    return ((0x0401 + k) | ((k & 1) << 15).astype(np.uint16)).view(np.float16).reshape(n_vp, V, IMG)


def location_table(V, LOC):
    """[V, V, LOC] fp32, every element distinct (a stand-in for features.build_loc_table: a wrong agent view must show)."""
    return (1.0 + np.arange(V * V * LOC, dtype=np.float64) / 64.0).astype(F32).reshape(V, V, LOC)


def sincos_constants(n):
    """[n, 4]: four distinct constants per row, distinct across rows, signs mixed."""
    k = np.arange(4 * n, dtype=np.float64).reshape(n, 4)
    return ((0.125 + k / 8.0) * np.where(k % 3 == 1, -1.0, 1.0)).astype(F32)


def sincos_of_angles(heading, elevation):
    """What the environment hands over (env.py:60-75): sin / cos in float64, stored as fp32."""
    h, e = np.asarray(heading, np.float64), np.asarray(elevation, np.float64)
    return np.stack((np.sin(h), np.cos(h), np.sin(e), np.cos(e)), axis=-1).astype(F32)


def gather_inputs(case, seed=0, angles=False):
    """Index-form inputs of one case with every index edge planted by position (rows permitting): vp < 0, view /
    cand_view below 0 and at or above V, a_num in {0, 1, A}, act over ACT_EDGES.  -> dict."""
    V, IMG, LOC, A, B = case
    rng = np.random.default_rng([V, IMG, LOC, A, B, seed])
    b = np.arange(B) + (V + IMG // 4 + LOC // 16 + A)                # (the one-row cases differ in what their row holds)
    vp = rng.integers(0, N_VP, B).astype(np.int32)
    vp[(b + seed) % 7 == 3] = -1
    view = rng.integers(0, V, B).astype(np.int32)
    for r, bad in ((0, -2), (2, V), (4, V + 5), (6, -1)):
        view[(b + seed) % 9 == r] = bad
    cand_view = rng.integers(0, V, (B, A)).astype(np.int32)
    flat = np.arange(B * A).reshape(B, A) + seed
    for r, bad in ((1, -3), (3, V), (5, V + 2)):
        cand_view[flat % 7 == r] = bad
    a_num = np.choose((b + seed) % 4, [np.zeros(B, int), np.ones(B, int), np.full(B, A), rng.integers(1, A + 1, B)])
    a_num = a_num.astype(np.int32)
    act = np.choose((b // 4 + b + seed) % 8, [np.full(B, -1), np.zeros(B, int), np.ones(B, int), a_num - 1, a_num,
                                              np.full(B, A), np.full(B, A + 3), rng.integers(0, A + 1, B)]).astype(np.int32)
    if angles:
        sincos = sincos_of_angles(rng.uniform(-np.pi, np.pi, (B, A)), rng.uniform(-np.pi / 2, np.pi / 2, (B, A)))
    else:
        sincos = sincos_constants(B * A).reshape(B, A, 4)
    # the single-row entry of the speaker: one (view, sin/cos, action) per row
    return dict(table16=feature_table16(V, IMG), loc=location_table(V, LOC), vp=vp, view=view, cand_view=cand_view,
                sincos=sincos, a_num=a_num, act=act, path_view=np.ascontiguousarray(cand_view[:, A - 1]),
                path_sincos=np.ascontiguousarray(sincos[:, A - 1]), path_act=np.where((b + seed) % 3 == 0, b % 2 - 1, 1 + b % 3).astype(np.int32))


def _clamp(i, n):
    return np.clip(i, 0, n - 1)


def model_panorama(table, loc, vp, view):
    """sf_gather_panorama: [B, V, IMG + LOC] = table[vp[b]] || loc[clamp(view[b])]; vp < 0 => zeros."""
    X = np.concatenate((table[np.maximum(vp, 0)].astype(F32), loc[_clamp(view, loc.shape[0])]), axis=2)
    X[vp < 0] = 0.0
    return X


def _candidate_rows(table, vp, cand_view, sincos, LOC):
    """[.., IMG + LOC] = table[vp, clamp(cand_view)] || each of sin h, cos h, sin e, cos e repeated LOC / 4 times."""
    assert LOC % 4 == 0
    V = table.shape[1]
    img = table[np.maximum(vp, 0).reshape(vp.shape + (1,) * (cand_view.ndim - vp.ndim)), _clamp(cand_view, V)].astype(F32)
    return np.concatenate((img, np.repeat(sincos, LOC // 4, axis=-1)), axis=-1)


def model_candidates(table, vp, cand_view, sincos, a_num, LOC):
    """sf_gather_candidates -> (all_u [B, A, F], is_valid [B, A]): row 0 (stop), rows >= a_num[b] and rows of vp < 0 are
    zero; is_valid = a < a_num[b]."""
    B, A = cand_view.shape
    U = _candidate_rows(table, vp, cand_view, sincos, LOC)
    a = np.arange(A)[None, :]
    U[(a == 0) | (a >= a_num[:, None]) | (vp < 0)[:, None]] = 0.0
    return U, (a < a_num[:, None]).astype(F32)


def model_actions(table, vp, cand_view, sincos, a_num, act, LOC, out=None):
    """sf_gather_actions / sf_gather_actions_ld: row b = candidate clamp(act[b]) of sample b; zeros for act <= 0, a
    (clamped) action at or behind a_num[b], vp < 0.  `out` [B, ld] (poisoned): columns >= F keep their contents."""
    B, A = cand_view.shape
    U = model_candidates(table, vp, cand_view, sincos, a_num, LOC)[0]
    rows = U[np.arange(B), _clamp(act, A)]
    rows[act <= 0] = 0.0
    if out is None:
        return rows
    out = out.copy()
    out[:len(rows), :rows.shape[1]] = rows
    return out


def model_path_actions(table, vp, act_view, sincos, act, LOC, out):
    """sf_gather_path_actions: row n of out [N, ld] = table[vp[n], clamp(act_view[n])] || sin/cos groups where
    act[n] > 0 and vp[n] >= 0, zeros elsewhere; columns >= IMG + LOC keep their contents."""
    rows = _candidate_rows(table, vp, act_view, sincos, LOC)
    rows[(act <= 0) | (vp < 0)] = 0.0
    out = out.copy()
    out[:len(rows), :rows.shape[1]] = rows
    return out


def gather_edges(case, seed=0):
    """The index edges the inputs of `case` hold, as a set of names (coverage: test_mover_cases_host.py)."""
    V, IMG, LOC, A, B = case
    d = gather_inputs(case, seed)
    e = set()
    live = d['vp'] >= 0
    if (~live).any():
        e.add('vp<0')
    for name, v in (('view', d['view'][live]), ('cand_view', d['cand_view'][live]), ('path_view', d['path_view'][live])):
        if (v < 0).any():
            e.add(name + '<0')
        if (v >= V).any():
            e.add(name + '>=V')
    for k, val in (('0', 0), ('1', 1), ('A', A)):
        if (d['a_num'] == val).any():
            e.add('a_num=' + k)
    an = d['a_num']
    for name, val in zip(ACT_EDGES, (-1, 0, 1, an - 1, an, A, A + 3)):
        if ((d['act'] == val) & live).any():
            e.add('act=' + name)
    if (d['path_act'] <= 0).any():
        e.add('path_act<=0')
    if ((d['path_act'] > 0) & live).any():
        e.add('path_act>0')
    return e


# ==================================================================================================== row movers
RowCase = namedtuple('RowCase', 'w n lds ldd pattern')
ROW_PATTERNS = ('neg', 'perm', 'repeat', 'ends')
ROW_W, ROW_N = (4, 8, 80, 512, 516), (1, 63, 257)


def _row_cases():
    out = []
    for i, (w, n) in enumerate(product(ROW_W, ROW_N)):
        for j in range(2):
            out.append(RowCase(w, n, w + 4 * j, w + 4 * ((i + j) & 1), ROW_PATTERNS[(i + 2 * j + i // 4) % 4]))
    return out


ROW_CASES = _row_cases()
ROW_BIG = RowCase(2052, 2049, 2056, 2052, 'perm')                  # n * w / 4 = 1 051 137 > GRID_PASS


def counting(rows, ld, w, start=1.0):
    """[rows, ld]: element (r, c < w) counts from `start` (exact in fp32), the padding columns hold NaN (read them and
    fail)."""
    a = np.full((rows, ld), np.nan, F32)
    a[:, :w] = (start + np.arange(rows * w, dtype=np.float64)).reshape(rows, w)
    return a


def row_indices(case, scatter, seed=0):
    """(idx [n] int32, pool rows): gather reads pool rows idx, scatter writes them (distinct where >= 0)."""
    w, n, lds, ldd, pattern = case
    rng = np.random.default_rng([w, n, lds, ldd, seed, int(scatter)])
    pool = n + 3
    if pattern == 'neg':
        idx = np.full(n, -1)
    elif pattern == 'perm' or (pattern == 'repeat' and scatter):
        idx = rng.permutation(pool)[:n]
        idx[np.arange(n) % 4 == 1] = -1
    elif pattern == 'repeat':
        idx = rng.integers(0, max(pool // 4, 1), n)
    else:                                                            # the first and the last pool row
        idx = rng.permutation(np.arange(1, pool - 1))[:n]
        idx[0] = pool - 1
        if n > 1:
            idx[-1] = 0
        elif (w // 4 + seed) % 2:
            idx[0] = 0
    return idx.astype(np.int32), pool


def model_gather_rows(src, idx, w, dst):
    """dst[i, :w] = src[idx[i], :w], idx < 0 => zeros; every other element of dst keeps its contents."""
    out = dst.copy()
    out[:len(idx), :w] = np.where((idx >= 0)[:, None], src[np.maximum(idx, 0), :w], F32(0.0))
    return out


def model_scatter_rows(src, idx, w, dst):
    """dst[idx[i], :w] = src[i, :w], idx < 0: row skipped (the idx >= 0 distinct)."""
    live = idx >= 0
    assert len(set(idx[live].tolist())) == int(live.sum()), 'scatter indices race'
    out = dst.copy()
    out[idx[live], :w] = src[:len(idx)][live, :w]
    return out


MoveCase = namedtuple('MoveCase', 'n moves')                       # moves: ((w, lds, ldd, scatter, pattern), ..)
MOVE_CASES = [
    MoveCase(1, ((8, 8, 12, 0, 'ends'),)),
    MoveCase(63, ((516, 520, 516, 1, 'perm'),)),
    MoveCase(257, ((80, 80, 84, 0, 'repeat'),)),
    MoveCase(1, ((4, 4, 4, 0, 'ends'), (80, 84, 80, 1, 'perm'), (512, 512, 516, 0, 'neg'), (516, 516, 516, 1, 'ends'))),
    MoveCase(63, ((512, 516, 512, 1, 'perm'), (4, 8, 4, 0, 'repeat'), (516, 516, 520, 0, 'perm'), (8, 8, 8, 1, 'neg'))),
    MoveCase(257, ((4, 4, 8, 1, 'ends'), (516, 520, 516, 0, 'ends'), (80, 80, 80, 1, 'perm'), (512, 512, 512, 0, 'repeat'))),
]
assert all(len(c.moves) in (1, ROW_MOVES_MAX) for c in MOVE_CASES)


def move_buffers(case, k, seed=0):
    """(src, dst, idx, w, scatter) of move k of a sf_move_rows case; model_gather_rows / model_scatter_rows give the result."""
    w, lds, ldd, scatter, pattern = case.moves[k]
    idx, pool = row_indices(RowCase(w, case.n, lds, ldd, pattern), bool(scatter), seed + k)
    src = counting(case.n if scatter else pool, lds, w, start=1.0 + 4096.0 * k)
    dst = poison(pool if scatter else case.n, ldd)
    return src, dst, idx, w, scatter


# =================================================================================================== plain movers
TRANSPOSE_CASES = [(1, 1), (1, 33), (31, 32), (32, 32), (33, 31), (64, 65), (100, 2176)]
EMBED_CASES = [(E, B) for E in (4, 32, 300) for B in (1, 100)]
EMBED_BIG = (4, GRID_PASS + 24)                                     # B * E / 4 > GRID_PASS
EMBED_VOCAB = 7
FILL_N = (0, 1, 255, 256, 257, GRID_PASS + 1)
DropCase = namedtuple('DropCase', 'p B N lds ldd col0 row0')
DROP_CASES = [DropCase(*c) for c in (
    (0.0, 3, 300, 304, 308, 0, 0), (0.0, 5, 1, 2, 3, 40, 17),
    (0.2, 3, 300, 308, 304, 0, 17), (0.2, 7, 1, 3, 2, 40, 0), (0.2, 4, 300, 301, 303, 40, 17),
    (0.5, 3, 300, 304, 301, 40, 0), (0.5, 9, 1, 5, 2, 0, 17), (0.5, 2, 300, 302, 310, 0, 0),
)]
DROP_BIG = DropCase(0.5, 3500, 300, 301, 302, 40, 17)               # B * N = 1 050 000 > GRID_PASS
DROP_SEED, DROP_STREAM = 0xC0FFEE, 5


def model_transpose(src):
    return np.ascontiguousarray(src.T)


def embedding_indices(E, B, vocab=EMBED_VOCAB):
    """[B] int64: 0 and vocab - 1 present (B permitting), repeats among the rest."""
    idx = np.random.default_rng([E, B]).integers(0, vocab, B).astype(np.int64)
    idx[0] = vocab - 1
    if B > 1:
        idx[-1] = 0
        idx[B // 2] = idx[B // 2 - 1]
    return idx


def model_embedding(table, idx):
    return table[idx]


def dropout_mask(p, rows, col0, N, seed=DROP_SEED, stream=DROP_STREAM):
    """The multiplicative mask [len(rows), N] of columns col0 .. col0 + N - 1 for GLOBAL rows `rows`: 0 or 1 / (1 - p) in
    fp32.  p travels through the ABI as a float (sf_dropout.p) and the threshold is formed from that float."""
    from oracle import rng as orng
    p32 = float(F32(p))
    return orng.dropout_mask(seed, stream, np.asarray(rows), col0 + N, p32)[:, col0:]


def model_dropout_copy(src, case, dst):
    """dst[b, :N] = keep ? src[b, :N] * scale : +0; columns >= N of dst keep their contents."""
    p, B, N, lds, ldd, col0, row0 = case
    m = dropout_mask(p, row0 + np.arange(B), col0, N)
    out = dst.copy()
    out[:, :N] = np.where(m != 0, src[:, :N] * m, F32(0.0))
    return out


# ====================================================================================== scoring-backward reducers
REDUCER_B = (1, 15, 16, 17, 48, 49, 64, 65, 193, 256, 257)        # the entry has no batch limit: none is dropped
REDUCER_D = (32, 64, 68)
REDUCER_A, REDUCER_F = 3, 8
Reducer = namedtuple('Reducer', 'U dlogit w wt t_a g0 grads')     # w = (w_h, b_h, w_a, b_a, w_out, b_out)


def reducer_case(B, D, seed=0):
    """The exact family of tests/attention_cases.py (identity rows in wt, dyadic values) carried to the three
    small-parameter gradients of sf_eltwise_prod_scoring_bwd:
        dc[b] = sum_a dlogit[b, a]                       dr[b] = sum_a dlogit[b, a] U[b, a]
        dwt[b, n] = dr[b] . w_a[n] + dc[b] b_a[n]        (w_a holds one 1 per row: dwt[b, n] = dr[b, n % F] + ..)
        b_a += sum_b dc[b] wt[b]     b_out += sum_b dc[b]     w_out += sum_b dwt[b] * t_a[b]
    Every operand is a small integer or a small integer over 2 or 4, so every sum is exact in fp32 in any order
    (asserted).  The gradients start from g0 != 0: an overwrite shows."""
    A, F = REDUCER_A, REDUCER_F
    rng = np.random.default_rng([B, D, seed, 31])
    U = rng.integers(-3, 4, (B, A, F)).astype(F32)
    dlogit = (rng.integers(-4, 5, (B, A)) / 2.0).astype(F32)
    w_a = np.zeros((D, F), F32)
    w_a[np.arange(D), np.arange(D) % F] = 1.0
    b_a = rng.integers(-2, 3, D).astype(F32)
    w_out = (rng.choice([-1.0, 1.0], D) * 2.0 ** rng.integers(0, 2, D)).astype(F32)
    w_h = np.zeros((D, D), F32)
    w_h[np.arange(D), np.arange(D)[::-1]] = 1.0
    wt = np.zeros((B, D), F32)
    wt[np.arange(B), np.arange(B) % D] = 2.0 ** rng.integers(-1, 2, B)
    t_a = rng.integers(-3, 4, (B, D)).astype(F32)
    g0 = dict(b_a=(5.0 + np.arange(D) % 3).astype(F32), b_out=np.asarray([-9.0], F32), w_out=(np.arange(D) % 5 - 7.0).astype(F32)[None, :])
    f8 = np.float64
    dc = dlogit.astype(f8).sum(1)
    dr = np.einsum('ba,baf->bf', dlogit.astype(f8), U.astype(f8))
    dwt = dr @ w_a.astype(f8).T + dc[:, None] * b_a.astype(f8)[None, :]
    g = dict(b_a=g0['b_a'] + (dc[:, None] * wt).sum(0), b_out=g0['b_out'] + dc.sum(),
             w_out=g0['w_out'] + (dwt * t_a).sum(0)[None, :])
    # exact in fp32 in any order: every term is a multiple of 2^-3 and the sum of the magnitudes stays below 2^20
    mags = max(np.abs(dc[:, None] * wt).sum(0).max(), np.abs(dc).sum(), np.abs(dwt * t_a).sum(0).max())
    assert mags + 16 < 2 ** 20 and all(np.array_equal(v * 8, np.round(v * 8)) for v in g.values())
    grads = {k: v.astype(F32) for k, v in g.items()}
    assert all(np.array_equal(grads[k].astype(f8), g[k]) for k in g)
    return Reducer(U, dlogit, (w_h, np.zeros(D, F32), w_a, b_a, w_out[None, :].copy(), np.zeros(1, F32)), wt, t_a, g0, grads)


# =========================================================================================================== Adam
ADAM_N = (1, 2, 3, 4, 5, 7, 1023, 4 * GRID_PASS + 5)              # the last: 1 048 577 float4 and a tail of 1
ADAM_WD = (0.0, 5e-4)
ADAM_STEPS = (1, 2, 1000)
ADAM_HYPER = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)      # train.py:263-268


def adam_state(n, seed=0):
    """(p, g, m, v) fp32 by element class k = index % 6, so that every step stays near lr and 4 e32 stays far below one
    step (an element left unstepped must show):
        0, 2   a usual gradient, m ~ 0.1, v ~ 1e-2 (0.3 + |N(0, 1)|)^2: no quotient far above 1
        1      g an exact zero, usual moments (m decays, p still moves)
        3      g an exact zero, v so near zero that eps decides the quotient (sqrt(v) <= 1e-10), m ~ 1e-8
        4      g an exact zero, v exactly zero, m ~ 1e-8: the quotient is m / eps
        5      a usual gradient onto m ~ 1e-8 and v at / near zero (what a first step sees)"""
    rng = np.random.default_rng([n, seed, 47])
    k = np.arange(n) % 6
    p = rng.standard_normal(n).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    g[(k == 1) | (k == 3) | (k == 4)] = 0.0
    m = (0.1 * rng.standard_normal(n)).astype(F32)
    quiet = (k == 3) | (k == 4) | (k == 5)
    m[quiet] = (1e-8 * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)[quiet]
    v = ((0.3 + np.abs(rng.standard_normal(n))) ** 2 * 1e-2).astype(F32)
    tiny = (k == 3) | (k == 5)
    v[tiny] = (10.0 ** rng.uniform(-30, -20, n)).astype(F32)[tiny]
    v[(k == 4) | (np.arange(n) % 12 == 5)] = 0.0
    return p, g, m, v


def model_adam(p, g, m, v, step, wd, dtype=np.float64, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """One torch.optim.Adam step (L2 weight decay in the gradient, 1-based `step`, no amsgrad) in `dtype`, in the
    operation order of torch's single-tensor implementation; the hyper-parameters stay Python floats.  -> (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    t = dtype
    if wd != 0:
        g = g + t(wd) * p
    m = m + t(1 - beta1) * (g - m)                                    # lerp, weight < 0.5
    v = v * t(beta2) + (t(1 - beta2) * g) * g                         # mul_ then addcmul_
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = np.sqrt(v) / t(np.sqrt(bc2)) + t(eps)
    p = p + (t(-(lr / bc1)) * m) / denom                              # addcdiv_
    return p, m, v


def adam_coef(step, lr=1e-4, beta1=0.9, beta2=0.999):
    """coef[0..1] of sf_adam_step_dev: the two step-dependent constants in double, rounded to fp32 once."""
    return F32(lr / (1.0 - beta1 ** step)), F32(1.0 / np.sqrt(1.0 - beta2 ** step))


def adam_within(got, r, f, what=''):
    """The rule of tests/grad_compare.py with an elementwise floor: |got - r| <= max(4 max|f - r|, two fp32 ulps of
    |r|).  -> (e, e32, share of the bound used); raises naming the first element out of bound."""
    got, r, f = (np.asarray(a, np.float64) for a in (got, r, f))
    assert got.shape == r.shape == f.shape, (what, got.shape, r.shape, f.shape)
    assert np.isfinite(got).all(), what + ': non-finite'
    e32 = float(np.abs(f - r).max())
    bound = np.maximum(4.0 * e32, 2.0 * np.spacing(np.abs(r).astype(F32)).astype(np.float64))
    d = np.abs(got - r)
    bad = np.flatnonzero(d > bound)
    assert len(bad) == 0, '%s: %d elements out of bound, first %d: got %r, want %r, |d| %.3e > %.3e (e32 %.3e)' % (
        what, len(bad), bad[0], got[bad[0]], r[bad[0]], d[bad[0]], bound[bad[0]], e32)
    return float(d.max()), e32, float((d / bound).max())
