"""Shapes, inputs and float64 references for tests/test_gpu_attention_dispatch.py (checked on the host by
tests/test_attention_cases_host.py): the row-set kernels of csrc/sf_attention.hip -- visual attention, text attention,
candidate scoring -- one kernel at a time, at every edge of their dispatch and of their bodies.

Two families of inputs:

  * selection (exact).  In sample b ONE designated row outscores every other row by more than 200, so expf of the
    difference is exactly 0 in fp32, the softmax is exactly one-hot and the output is exactly that row, all 24 mantissa
    bits of it, whatever the summation order.  The query is 512 at one "hot" column (a chunk edge of the row: first,
    last, around float4 63|64 and 511|512) plus noise of +-2^-9 / 2^-10 everywhere; the rows are full-mantissa numbers of
    magnitude [0.5, 2) whose hot column is +[1.5, 2) in the designated row and +-[0.5, 1) in the others: the designated
    score is >= 768 - 9, every other <= 512 + 9.  Sample b designates row b mod V (b mod L), so with B >= V every row
    of every wave and of each split group is designated once.  For the entries that form the query themselves the
    weights hold 0 / 2^e only, so every product in front of the kernel is an exact copy (the GEMM kernels are exact on
    such operands: tests/test_gpu_gemm_dispatch.py).  Scoring: r is one-hot 2^e, the constant one exact product plus an
    integer, so every logit is a single product plus a constant, rounded once.
  * dense (float64 reference).  Badly scaled (every 7th column four times larger, a common offset), asymmetric rows (row l
    scaled by 1 + l / 50), a query whose columns follow another period (5): no swap of rows, columns or chunks cancels.
    Score spreads are a few units, so no weight underflows.  Each formula below takes a dtype: float64 is the reference,
    the float32 evaluation of the SAME formula on the same inputs is the yardstick e32.

`layout` / `outside_is_untouched` (tests/gemm_cases.py) pad strided vectors with NaN (inputs) or a sentinel (outputs)."""
from collections import namedtuple

import numpy as np

from tests.gemm_cases import SENTINEL, TAIL_ROWS, layout, outside_is_untouched          # noqa: F401

# ------------------------------------------------------------------------------------------ constants
# (speaker_follower_amd/csrc/sf_attention_plan.h unless another file is named; the symbol each value mirrors)
VIS_CPL, VIS_RPW, VIS_NW = 9, 3, 12           # VIS_CPL, VIS_RPW, VIS_NW   float4 chunks per lane, rows per wave, waves
VSP_G = 2                                     # VSP_G  SF_VIS_GROUPS: workgroups per sample of the split forward
VSP_RPG = VIS_NW // VSP_G * VIS_RPW           # VSP_RPG  rows per group = 18
VIS_SPLIT_MAX_B = 256                         # VIS_SPLIT_MAX_B
TXT_CPL, TXT_NW = 2, 16                       # TXT_CPL, TXT_NW
TXT_RPW = (1, 5, 8)                           # text_rpw  (sf_attention.hip: text_attn_launch): L <= 16 RPW
SC_CPL, SC_NW = 9, 16                         # SC_CPL, SC_NW
CG_ROWS, CG_THREADS, CG_LDS = 10, 1024, 64 * 1024     # CG_ROWS, ctx_grad_supported  ctx_grad_kernel

V_MAX = min(VIS_RPW * VIS_NW, 64)             # pano_rows_fit  36
V_SPLIT_LO = (VSP_G - 1) * VSP_RPG            # in_split_range  the split forward runs for V_SPLIT_LO < V <= V_MAX
F_MAX = VIS_CPL * 256                         # row_width_fits  2304 (both CPL are 9)
H_MAX = TXT_CPL * 256                         # text_rows_fit  512
L_MAX = TXT_NW * TXT_RPW[-1]                  # TXT_MAX_L  128
A_MAX = SC_NW                                 # cand_rows_fit  16
SOFTMAX_HALF = 64                             # sf_attention.hip: text_attn_body   lane holds positions lane and lane + 64
SCORE_LOC_MULTIPLE = 16                       # cand_rows_fit  index form: LOC % 16 == 0

VIS_FWD, VIS_BWD, VIS_SPLIT, VIS_F64 = ('visual_attn_kernel<0>', 'visual_attn_kernel<1>', 'visual_attn_split_kernel',
                                        'visual_attn_split_f64_kernel')
TXT = 'text_attn_kernel<%d, MODE>'
SCORE_FWD, SCORE_BWD, CTX_GRAD_KERNEL = 'score_fwd_kernel', 'score_bwd_kernel', 'ctx_grad_kernel'
ATTENTION_KERNELS = ('visual_attn', 'text_attn', 'score_fwd', 'score_bwd', 'score_glue', 'ctx_grad')      # name prefixes


def half_name(kernel):
    """The name the profile reports for the binary16-table instantiation (SF_LAUNCH_H16 / SF_LAUNCH_H16_AS)."""
    return kernel[:-1] + ', true>' if kernel.endswith('>') else kernel + '<f16>'


def visual_fwd_kernel(V, B, workspace=True):
    """visual_attn (sf_attention.hip), forward: in_split_range."""
    return VIS_SPLIT if workspace and V_SPLIT_LO < V <= V_MAX and B <= VIS_SPLIT_MAX_B else VIS_FWD


def visual_f64_supported(V, B, F):
    """visual_attn_f64_supported (split_rows_fit), dense source."""
    return V_SPLIT_LO < V <= V_MAX and B <= VIS_SPLIT_MAX_B and F <= F_MAX and F % 4 == 0


def text_kernel(L):
    """text_attn_launch (text_rpw); None = SF_ERR_UNSUPPORTED."""
    for r in TXT_RPW:
        if L <= TXT_NW * r:
            return TXT % r
    return None


def ctx_grad_supported(S, L, H):
    """ctx_grad_supported."""
    n4 = H >> 2
    return (H % 4 == 0 and 1 <= n4 <= CG_THREADS and CG_THREADS % n4 == 0 and L <= (CG_THREADS // n4) * CG_ROWS and
            S * 2 * L * 4 <= CG_LDS)


# ---------------------------------------------------------------------------------------------- cases
Vis = namedtuple('Vis', 'kernel V B F')                    # dense source, forward
VisIndex = namedtuple('VisIndex', 'kernel V B IMG LOC')    # index form (one sample at vp = -1)
Txt = namedtuple('Txt', 'kernel L H B')
Score = namedtuple('Score', 'kernel A B F')
ScoreIndex = namedtuple('ScoreIndex', 'kernel A B IMG LOC')
Refusal = namedtuple('Refusal', 'entry what status dims')
CtxGrad = namedtuple('CtxGrad', 'L S runs')

F_EDGES = (4, 256, 260, 2052, 2176, 2300, 2304)            # n4 = 1, 64, 65, 513, 544, 575, 576
VIS_V = (1, 2, V_SPLIT_LO - 1, V_SPLIT_LO, V_SPLIT_LO + 1, V_SPLIT_LO + 2, V_MAX - 1, V_MAX)
VIS_B = (1, VIS_SPLIT_MAX_B - 1, VIS_SPLIT_MAX_B, VIS_SPLIT_MAX_B + 1)
TXT_L = (1, 2, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128)
TXT_H = (4, 252, 256, 260, 508, 512)
SCORE_A = (1, 2, A_MAX - 1, A_MAX)


def _vis(V, B, F):
    return Vis(visual_fwd_kernel(V, B), V, B, F)


VISUAL = ([_vis(V, 3, 260) for V in VIS_V] +                                        # the row-to-wave mapping
          [_vis(V_MAX, B, 64) for B in VIS_B] +                                     # the batch threshold of the split
          [_vis(V, 3, F) for F in F_EDGES for V in (V_SPLIT_LO, V_SPLIT_LO + 1, V_MAX)])    # the chunk bounds
VISUAL_INDEX = [VisIndex(visual_fwd_kernel(V, 4), V, 4, IMG, LOC)
                for IMG, LOC in ((8, 4), (252, 4), (2048, 128), (2176, 128)) for V in (5, V_SPLIT_LO + 1, V_MAX)]
# the backward (always un-split): the rows, then the chunks
VISUAL_BWD = ([Vis(VIS_BWD, V, 3, 260) for V in VIS_V] + [Vis(VIS_BWD, V_MAX, 3, F) for F in F_EDGES])
# the float64-score forward: only inside the split's range
VISUAL_F64 = [Vis(VIS_F64, V, 3, F) for V in (V_SPLIT_LO + 1, V_MAX) for F in (260, 2176)]
TEXT = [Txt(text_kernel(L), L, H, 3) for L in TXT_L for H in TXT_H]
SCORE = ([Score(SCORE_FWD, A, 3, 260) for A in SCORE_A] + [Score(SCORE_FWD, A, 3, F) for F in F_EDGES for A in (2, A_MAX)])
SCORE_INDEX = [ScoreIndex(SCORE_FWD, A, 5, IMG, LOC) for IMG, LOC in ((8, 16), (2048, 128), (2176, 128))
               for A in (1, A_MAX - 1, A_MAX)]

# one step past each limit: argument checking only (valid, finite inputs of the refused shape)
REFUSALS = [
    Refusal('visual', 'V = V_MAX + 1', 2, dict(V=V_MAX + 1, F=64)),
    Refusal('visual', 'F = F_MAX + 4', 2, dict(V=4, F=F_MAX + 4)),
    Refusal('visual', 'F % 4 != 0', 2, dict(V=4, F=258)),
    Refusal('visual', 'ldo % 4 != 0', 2, dict(V=4, F=64, ldo=66)),
    Refusal('text', 'L = L_MAX + 1', 2, dict(L=L_MAX + 1, H=64)),
    Refusal('text', 'H = H_MAX + 4', 2, dict(L=4, H=H_MAX + 4)),
    Refusal('score', 'A = A_MAX + 1', 2, dict(A=A_MAX + 1, F=64)),
    Refusal('score', 'F = F_MAX + 4', 2, dict(A=2, F=F_MAX + 4)),
    Refusal('score', 'F % 4 != 0', 2, dict(A=2, F=258)),
]

# follower training passes around ctx_grad_supported at H = 512: L <= 80 and S L <= 8192
CTX_GRAD = [CtxGrad(80, 102, True), CtxGrad(80, 103, False), CtxGrad(81, 5, False)]


def boundaries():
    """Every boundary of the dispatch and the bodies as (name, table, field(s), value below, value above), derived from
    the constants alone; `above` None: the far side is a refusal (an entry of REFUSALS for the same kernel -- the first
    word of the name -- with a larger value of the field)."""
    out = [('visual split V', VISUAL, 'V', V_SPLIT_LO, V_SPLIT_LO + 1),
           ('visual split nearly empty group', VISUAL, 'V', V_SPLIT_LO + 1, V_SPLIT_LO + 2),
           ('visual V_MAX', VISUAL, 'V', V_MAX, None),
           ('visual smallest V', VISUAL, 'V', 1, 2),
           ('visual split B', VISUAL, 'B', VIS_SPLIT_MAX_B, VIS_SPLIT_MAX_B + 1),
           ('visual backward V_MAX', VISUAL_BWD, 'V', V_MAX - 1, V_MAX),
           ('score A_MAX', SCORE, 'A', A_MAX, None), ('score A', SCORE, 'A', A_MAX - 1, A_MAX),
           ('text L_MAX', TEXT, 'L', L_MAX, None), ('text softmax halves', TEXT, 'L', SOFTMAX_HALF, SOFTMAX_HALF + 1),
           ('text H_MAX', TEXT, 'H', H_MAX, None), ('text one chunk per lane', TEXT, 'H', 256, 260)]
    for r in TXT_RPW[:-1]:
        out.append(('text RPW %d' % r, TEXT, 'L', TXT_NW * r, TXT_NW * r + 1))
    for table, name in ((VISUAL, 'visual'), (VISUAL_BWD, 'visual backward'), (SCORE, 'score')):
        if table is VISUAL_BWD:            # (its refusal is the forward's: the backward only runs behind a forward)
            out.append((name + ' F_MAX', table, 'F', F_MAX - 4, F_MAX))
        else:
            out.append((name + ' F_MAX', table, 'F', F_MAX, None))
        out.append((name + ' last chunk holds one lane', table, 'F', 4 * (64 * (VIS_CPL - 1) + 1), F_MAX - 4))
        out.append((name + ' one chunk', table, 'F', 4 * 64, 4 * 65))
        out.append((name + ' one float4', table, 'F', 4, 4 * 64))
    return out


# ----------------------------------------------------------------------------------------- references
def _softmax(s, axis):
    m = s.max(axis, keepdims=True)
    e = np.exp(s - m)
    return e / e.sum(axis, keepdims=True)


def visual_fwd(X, q, dtype=np.float64):
    """alpha = softmax_v(X . q), out = alpha . X   (visual_attn_body<0>)."""
    X, q = X.astype(dtype), q.astype(dtype)
    alpha = _softmax(np.einsum('bvf,bf->bv', X, q), 1)
    return alpha, np.einsum('bv,bvf->bf', alpha, X)


def visual_bwd(X, alpha, dout, dtype=np.float64):
    """w_v = alpha_v (d_v - sum alpha d), d_v = x_v . dout;  dq = sum w_v x_v   (visual_attn_body<1>)."""
    X, alpha, dout = X.astype(dtype), alpha.astype(dtype), dout.astype(dtype)
    d = np.einsum('bvf,bf->bv', X, dout)
    w = alpha * (d - (alpha * d).sum(1, keepdims=True))
    return np.einsum('bv,bvf->bf', w, X)


def text_fwd(ctx, t, mask=None, dtype=np.float64):
    """s_l = ctx_l . t (masked: -inf), alpha = softmax, wc = sum alpha_l ctx_l   (text_attn_body<., 0>)."""
    ctx, t = ctx.astype(dtype), t.astype(dtype)
    s = np.einsum('blh,bh->bl', ctx, t)
    if mask is not None:
        s = np.where(mask.astype(bool), dtype(-np.inf), s)
    alpha = _softmax(s, 1)
    return alpha, np.einsum('bl,blh->bh', alpha, ctx)


def text_bwd(ctx, t, alpha, dwc, dctx0=None, dtype=np.float64):
    """d_l = ctx_l . dwc, ds_l = alpha_l (d_l - sum alpha d), dt = sum ds_l ctx_l, dctx_l = dctx0_l + alpha_l dwc + ds_l t
    (text_attn_body<., 1>).  Returns (dt, dctx, ds)."""
    ctx, t, alpha, dwc = (a.astype(dtype) for a in (ctx, t, alpha, dwc))
    d = np.einsum('blh,bh->bl', ctx, dwc)
    ds = alpha * (d - (alpha * d).sum(1, keepdims=True))
    dt = np.einsum('bl,blh->bh', ds, ctx)
    dctx = alpha[:, :, None] * dwc[:, None, :] + ds[:, :, None] * t[:, None, :]
    if dctx0 is not None:
        dctx = dctx0.astype(dtype) + dctx
    return dt, dctx, ds


def score_fwd(U, r, cst, dtype=np.float64):
    """logit[b, a] = u_a . r[b] + cst[b]   (score_fwd_kernel; cst = wt . b_a + b_out)."""
    return np.einsum('baf,bf->ba', U.astype(dtype), r.astype(dtype)) + cst.astype(dtype)[:, None]


def score_const(wt, b_a, b_out, dtype=np.float64):
    return wt.astype(dtype) @ b_a.astype(dtype) + dtype(b_out)


def score_bwd(U, dlogit, dtype=np.float64):
    """dr[b] = sum_a dlogit[b, a] u_a, dc[b] = sum_a dlogit[b, a]   (score_bwd_kernel)."""
    dlogit = dlogit.astype(dtype)
    return np.einsum('ba,baf->bf', dlogit, U.astype(dtype)), dlogit.sum(1)


# ------------------------------------------------------------------------------------------ tolerance
FLOOR, CEILING, K = 2e-6, 1e-4, 4.0          # tests/grad_compare.py's floor, the project's TOL, another summation order


def rel_err(got, ref64):
    """max |got - ref64| / max |ref64| (the tensor's own scale)."""
    ref64 = np.asarray(ref64, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref64).max() / max(float(np.abs(ref64).max()), 1e-300))


def bound(e32):
    return min(max(K * e32, FLOOR), CEILING)


# ------------------------------------------------------------------------------------------- operands
HOT, GAP = 512.0, 200.0


def full_mantissa(rng, *shape, bits=24, lo=0.5):
    """float32 +-[lo, 2 lo) x {1, 2} using all `bits` mantissa bits (24: float32; 11: also exact in binary16)."""
    m = rng.integers(2 ** (bits - 1), 2 ** bits, shape).astype(np.float64) * 2.0 ** -bits          # [0.5, 1)
    v = m * (2.0 * lo) * rng.choice([1.0, 2.0], shape) * rng.choice([-1.0, 1.0], shape)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def edge_columns(n, F):
    """n column indices < F, starting with the edges of the chunk ownership (lane + 64 i owns float4 c): the last and
    first column, float4 63 | 64 and 511 | 512, the last float4's first column; then a stride-7 walk."""
    base = [F - 1, 0, 255, 256, 2047, 2048, F - 4, 4 * 64 * (VIS_CPL - 1) - 1]
    cols = [min(max(c, 0), F - 1) for c in base]
    k = 0
    while len(cols) < n:
        cols.append((7 * k + 3) % F)
        k += 1
    return np.asarray(cols[:n], np.int64)


def _hot_rows(rng, B, R, F, f0, sel, bits):
    """[B, R, F] full-mantissa rows whose column f0[b] is +[1.5, 2) in row sel[b] and +-[0.5, 1) in the others."""
    X = full_mantissa(rng, B, R, F, bits=bits)
    other = full_mantissa(rng, B, R, bits=bits)
    other = np.where(np.abs(other) >= 1.0, other * np.float32(0.5), other)                          # +-[0.5, 1)
    top = (rng.integers(3 * 2 ** (bits - 2), 2 ** bits, B).astype(np.float64) * 2.0 ** (1 - bits)).astype(np.float32)
    rows = np.arange(B)
    X[rows, :, f0] = other
    X[rows, sel, f0] = top                                                                          # [1.5, 2)
    return X


def _hot_query(rng, B, F, f0, groups=4):
    """q[b, f] = 512 [f == f0[b]] + wn[f] tn[b, f % groups], wn = +-2^-9 / 2^-10, tn = +-1: exact in float32, and a sum
    of (at most) two exact products when formed by a product against 0 / 2^e weights.  Returns (q, wn, tn)."""
    wn = (rng.choice([-1.0, 1.0], F) * 2.0 ** rng.choice([-9.0, -10.0], F)).astype(np.float32)
    tn = rng.choice([-1.0, 1.0], (B, groups)).astype(np.float32)
    q = wn[None, :] * tn[:, np.arange(F) % groups]
    q[np.arange(B), f0] += np.float32(HOT)
    return q.astype(np.float32), wn, tn


Selection = namedtuple('Selection', 'X q f0 sel wn tn')


def visual_selection(B, V, F, seed=0, hot=None, bits=24):
    """Rows X [B, V, F] and queries q [B, F] of the selection family: sample b designates row b mod V, through one of
    the first `hot` columns (index form: the image part; the location columns, |x| <= 1, only add noise)."""
    rng = np.random.default_rng([seed, B, V, F, 11])
    f0 = edge_columns(B, F if hot is None else hot)
    sel = np.arange(B) % V
    X = _hot_rows(rng, B, V, F, f0, sel, bits)
    q, wn, tn = _hot_query(rng, B, F, f0)
    return Selection(X, q, f0, sel, wn, tn)


def text_selection(B, L, H, seed=0):
    """Context rows [B, L, H] and targets t [B, H]: sample b designates position b mod L."""
    rng = np.random.default_rng([seed, B, L, H, 12])
    f0 = edge_columns(B, H)
    sel = np.arange(B) % L
    ctx = _hot_rows(rng, B, L, H, f0, sel, 24)
    t, wn, tn = _hot_query(rng, B, H, f0)
    return Selection(ctx, t, f0, sel, wn, tn)


def selection_is_one_hot(rows, q, sel, mask=None):
    """Whether every non-designated (unmasked) row's fp32 score lies GAP below the designated one -- under the worst
    case over summation orders: |score - exact| <= F eps sum |x q|."""
    x64, q64 = rows.astype(np.float64), q.astype(np.float64)
    s = np.einsum('brf,bf->br', x64, q64)
    slack = rows.shape[2] * 2.0 ** -23 * np.einsum('brf,bf->br', np.abs(x64), np.abs(q64))
    top = s[np.arange(len(sel)), sel] - slack[np.arange(len(sel)), sel]
    rest = s + slack
    rest[np.arange(len(sel)), sel] = -np.inf
    if mask is not None:
        rest = np.where(mask.astype(bool), -np.inf, rest)
    return bool((top - rest.max(1) >= GAP).all() if rows.shape[1] > 1 else True)


def round4(n):
    return (n + 3) // 4 * 4


VisualWeights = namedtuple('VisualWeights', 'h w_h b_h w_v b_v')


def visual_selection_weights(s, groups=4):
    """h [B, H], W_h [D, H], b_h, W_v [D, F] (H = D = round4(B) + groups) holding 0 / 2^e only, with
    (h W_h^T + b_h) W_v == s.q exactly: t_v[b, j] = [j == b] picks row j of W_v (512 at column f0[j]), the last `groups`
    entries of t_v carry tn and pick the noise rows; W_h is a scaled reversal, so t_v is a permuted, rescaled copy of h."""
    B, F = s.q.shape
    Bp = round4(B)
    D = Bp + groups
    t_v = np.zeros((B, D), np.float32)
    t_v[np.arange(B), np.arange(B)] = 1.0
    t_v[:, Bp:] = s.tn
    w_v = np.zeros((D, F), np.float32)
    w_v[np.arange(B), s.f0] = HOT
    cols = np.arange(F)
    w_v[Bp + cols % groups, cols] = s.wn
    scale = (2.0 ** ((np.arange(D) % 5) - 2)).astype(np.float32)
    perm = np.arange(D)[::-1]
    w_h = np.zeros((D, D), np.float32)
    w_h[np.arange(D), perm] = scale
    h = np.zeros((B, D), np.float32)
    h[:, perm] = t_v / scale[None, :]
    return VisualWeights(h, w_h, np.zeros(D, np.float32), w_v, np.zeros(D, np.float32))


def _rows_dense(rng, B, R, F):
    cols = np.arange(F)
    x = rng.standard_normal((B, R, F)) * (1.0 + 3.0 * (cols % 7 == 0))[None, None, :] + 0.25
    return (x * (1.0 + np.arange(R) / 50.0)[None, :, None]).astype(np.float32)


def _query_dense(rng, B, F, spread=0.77):
    return (rng.standard_normal((B, F)) * (spread * F ** -0.5) * ((1.0 + np.arange(F) % 5) / 3.0)[None, :]).astype(np.float32)


def visual_dense(B, V, F, seed=0, H=32, D=32):
    """(X, weights) of the dense family: the entry forms q = (h W_h^T + b_h) W_v, of the scale of `_query_dense`."""
    rng = np.random.default_rng([seed, B, V, F, 21])
    X = _rows_dense(rng, B, V, F)
    h = rng.standard_normal((B, H)).astype(np.float32)
    w_h = (rng.standard_normal((D, H)) * H ** -0.5).astype(np.float32)
    b_h = (rng.standard_normal(D) * 0.1).astype(np.float32)
    w_v = (rng.standard_normal((D, F)) * (0.7 * (F * D) ** -0.5) * ((1.0 + np.arange(F) % 5) / 3.0)[None, :]).astype(np.float32)
    return X, VisualWeights(h, w_h, b_h, w_v, (rng.standard_normal(D) * 0.1).astype(np.float32))


def visual_query(w, dtype=np.float32):
    """(t_v, q) of the weights on the host (what the entry's two products form)."""
    t_v = w.h.astype(dtype) @ w.w_h.astype(dtype).T + w.b_h.astype(dtype)
    return t_v, t_v @ w.w_v.astype(dtype)


def shift_scores(X, q, rows, by):
    """X with `by` added to the score of the given rows (a multiple of q added to them): the imbalanced split merge."""
    X = X.copy()
    unit = (q.astype(np.float64) / (q.astype(np.float64) ** 2).sum(1, keepdims=True))               # x . q = 1
    X[:, rows, :] = (X[:, rows, :].astype(np.float64) + by * unit[:, None, :]).astype(np.float32)
    return X


VisualBwdExact = namedtuple('VisualBwdExact', 'X alpha dout dq')


def visual_bwd_exact(B, V, F, seed=0):
    """Small-integer X (|x| <= 4), dyadic alpha (2^-1 .. 2^-4, or 0), dout with +-1 / +-2 at eight edge columns: every
    score gradient is an integer, w_v a multiple of 2^-8 and every partial sum of dq below 2^24 of that unit -- dq is
    exact in float32 in any summation order (asserted here)."""
    rng = np.random.default_rng([seed, B, V, F, 31])
    X = rng.integers(-4, 5, (B, V, F)).astype(np.float32)
    alpha = (2.0 ** -rng.integers(1, 5, (B, V)) * (rng.random((B, V)) < 0.8)).astype(np.float32)
    dout = np.zeros((B, F), np.float32)
    dout[:, edge_columns(8, F)] = rng.choice([-2.0, -1.0, 1.0, 2.0], (B, 8))      # (F = 4: the edges coincide)
    f64 = np.float64
    d = np.einsum('bvf,bf->bv', X.astype(f64), dout.astype(f64))
    w = alpha.astype(f64) * (d - (alpha.astype(f64) * d).sum(1, keepdims=True))
    assert float(np.einsum('bv,bvf->bf', np.abs(w), np.abs(X).astype(f64)).max()) < 2.0 ** 24 * 2.0 ** -8
    dq = np.einsum('bv,bvf->bf', w, X.astype(f64))
    out = dq.astype(np.float32)
    assert np.array_equal(out.astype(f64), dq) and np.array_equal(w * 256.0, np.rint(w * 256.0))
    return VisualBwdExact(X, alpha, dout, out)


def copy_weights(B, F, D=None):
    """0 / 1 weights around the visual backward: t_v [B, D] = identity rows (so the weight gradient t_v^T dq holds dq
    itself in its rows < B), W_v [D, F] with a single 1 per row at an edge column and W_h = identity [D, D] (so
    dh[:, d] = dq[:, cols[d]]).  Returns (t_v, w_h, w_v, cols)."""
    D = round4(max(B, 8)) if D is None else D
    t_v = np.zeros((B, D), np.float32)
    t_v[np.arange(B), np.arange(B)] = 1.0
    cols = edge_columns(D, F)
    w_v = np.zeros((D, F), np.float32)
    w_v[np.arange(D), cols] = 1.0
    return t_v, np.eye(D, dtype=np.float32), w_v, cols


def text_dense(B, L, H, seed=0):
    """ctx [B, L, H], t, dwc [B, H] and a non-zero initial dctx of the dense family."""
    rng = np.random.default_rng([seed, B, L, H, 22])
    ctx = _rows_dense(rng, B, L, H)
    t = _query_dense(rng, B, H)
    dwc = (rng.standard_normal((B, H)) * (1.0 + np.arange(H) % 3)[None, :]).astype(np.float32)
    dctx0 = rng.standard_normal((B, L, H)).astype(np.float32)
    return ctx, t, dwc, dctx0


MASKS = ('none', 'ragged', 'hole')


def text_mask(kind, B, L):
    """uint8 [B, L] (1 = masked) or None.  ragged: lengths L, 1, about L / 2, ... ; hole: one masked position in the
    middle of every row (L >= 3; shorter: the last position of row 1 only, rows must keep one live position)."""
    if kind == 'none':
        return None
    m = np.zeros((B, L), np.uint8)
    if kind == 'ragged':
        lens = [L, 1, (L + 1) // 2] + [max(1, L - b) for b in range(3, B)]
        for b in range(B):
            m[b, lens[b]:] = 1
    elif L >= 3:
        m[:, L // 2] = 1
    elif L == 2 and B > 1:
        m[1, 1] = 1
    return m


def neighbour_mask(L):
    """uint8 [L, L] for the selection family with B = L: in sample b the position behind the designated one is masked."""
    m = np.zeros((L, L), np.uint8)
    if L > 1:
        m[np.arange(L), (np.arange(L) + 1) % L] = 1
    return m


ScoreSel = namedtuple('ScoreSel', 'U h w r cst f0')          # w = (w_h, b_h, w_a, b_a, w_out, b_out)


def score_selection(B, A, F, seed=0, bits=24, U=None):
    """Candidates U [B, A, F] (full mantissa) and 0 / 2^e weights for which the entry forms r[b] = 2^e at column f0[b]
    (zero elsewhere) and the constant c[b] = 3 k_b - 7 (k_b a small integer): logit[b, a] = fl(2^e U[b, a, f0[b]] + c[b]),
    one product and one rounding.  D = H = round4(B + 1): wt[b, j] = +-2^k [j == b] picks row j of W_a, wt[b, B] = k_b
    meets the only non-zero of b_a."""
    rng = np.random.default_rng([seed, B, A, F, 13])
    if U is None:
        U = full_mantissa(rng, B, A, F, bits=bits)
    f0 = edge_columns(B, F)
    D = round4(B + 1)
    wt = np.zeros((B, D), np.float32)
    wt[np.arange(B), np.arange(B)] = rng.choice([-1.0, 1.0], B) * 2.0 ** rng.integers(-2, 3, B)
    kb = rng.integers(-3, 4, B).astype(np.float32)
    wt[:, B] = kb
    w_a = np.zeros((D, F), np.float32)
    w_a[np.arange(B), f0] = 2.0 ** rng.integers(-2, 3, B)
    b_a = np.zeros(D, np.float32)
    b_a[B] = 3.0
    w_out = (rng.choice([-1.0, 1.0], D) * 2.0 ** rng.integers(-1, 2, D)).astype(np.float32)
    t_a = wt / w_out[None, :]
    perm = np.arange(D)[::-1]
    w_h = np.zeros((D, D), np.float32)
    w_h[np.arange(D), perm] = 1.0
    h = np.zeros((B, D), np.float32)
    h[:, perm] = t_a
    r = np.zeros((B, F), np.float32)
    r[np.arange(B), f0] = wt[np.arange(B), np.arange(B)] * w_a[np.arange(B), f0]
    cst = (3.0 * kb - 7.0).astype(np.float32)
    w = (w_h, np.zeros(D, np.float32), w_a, b_a, w_out[None, :].copy(), np.asarray([-7.0], np.float32))
    return ScoreSel(U, h, w, r, cst, f0)


def score_selection_logits(U, r, cst, f0):
    """The exact logits: one product, the constant added in one rounding."""
    rows = np.arange(U.shape[0])
    prod = U[rows, :, f0].astype(np.float64) * r[rows, f0].astype(np.float64)[:, None]
    return (prod + cst.astype(np.float64)[:, None]).astype(np.float32)


def score_dense(B, A, F, seed=0, H=32, D=32):
    """(U, h, weights) of the dense family."""
    rng = np.random.default_rng([seed, B, A, F, 23])
    U = _rows_dense(rng, B, A, F)
    h = rng.standard_normal((B, H)).astype(np.float32)
    w = ((rng.standard_normal((D, H)) * H ** -0.5).astype(np.float32), (rng.standard_normal(D) * 0.1).astype(np.float32),
         (rng.standard_normal((D, F)) * (F ** -0.5) * ((1.0 + np.arange(F) % 5) / 3.0)[None, :]).astype(np.float32),
         (rng.standard_normal(D) * 0.1).astype(np.float32), (rng.standard_normal((1, D)) * D ** -0.5).astype(np.float32),
         (rng.standard_normal(1) * 0.1).astype(np.float32))
    return U, h, w


# ---------------------------------------------------------------------------------------- index form
def loc_table(V, LOC):
    """The location table [V, V, LOC] of a FeatureStore with V views (features.build_loc_table itself: no GPU needed)."""
    from speaker_follower_amd.features import build_loc_table
    return build_loc_table(V, LOC)


def dense_panorama(table, loc, vp, view):
    """[B, V, IMG + LOC]: table[vp] || loc[view]; all zero where vp < 0 (sf_pano)."""
    X = np.concatenate((table[np.maximum(vp, 0)].astype(np.float32), loc[view]), axis=2)
    X[vp < 0] = 0.0
    return X


def dense_candidates(table, vp, cand_view, sincos, a_num, LOC):
    """[B, A, IMG + LOC]: table[vp, cand_view] || sin/cos each repeated LOC / 4 times; row 0, rows >= a_num and rows of
    vp < 0 are zero (sf_cands)."""
    B, A = cand_view.shape
    img = table[np.maximum(vp, 0)[:, None], cand_view].astype(np.float32)
    U = np.concatenate((img, np.repeat(sincos, LOC // 4, axis=2)), axis=2)
    dead = (np.arange(A)[None, :] == 0) | (np.arange(A)[None, :] >= a_num[:, None]) | (vp < 0)[:, None]
    U[dead] = 0.0
    return U
