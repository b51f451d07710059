"""Shapes, inputs and models for tests/test_gpu_lstm_steps.py (checked on the host by tests/test_lstm_step_cases_host.py):
the per-step LSTM kernels -- lstm_step_fused_kernel<8|16>, lstm_step_wide_kernel<2|4>, lstm_bwd_step_fused_kernel<8|16>
(csrc/sf_gemm.hip), lstm_pw_fwd_kernel<KS>, lstm_pw_bwd_kernel (csrc/sf_pointwise.hip, csrc/sf_lstm_pw.h) -- one launch
at a time, at every edge of the two launchers' dispatch.

The mirror of the dispatch works on total = H/16 + ceil(I/16), the 16-wide chunks of the reduction: the 32-row kernel
for B > 16 (2 chunks per wave up to total 32, 4 up to 64), the 16-row kernel otherwise (8 chunks per K-slice up to total
32, 16 up to 64), nothing above 64.

Two input families.  EXACT: every gate row holds one weight +-1, operands lie on {0, 40}, biases and table rows on
{0, +-40} and only where the row's operand column is held at zero in that run, c0 on {0, +-64}: every pre-activation is
one term, the gates are 0.5 / 1 and 0 / +-1, c1 is exact and h1 is exact wherever c1 == 0 or |c1| >= 16; compared bit
for bit.  The encoder's recurrence starts from a zero state the entry fills itself, so there only step 0 is on the
lattice; its later steps go under the dense rule.  The exact backward is fed hand-made tapes (dyadic gates, c on
{0, +-32}, small-integer gradients, 0/1 selection rows in W_hh^T).  DENSE: seeded N(0, 1) operands, weights x H^-0.5
(peaky: x 8 more), against the float64 model under the project's rule (tests/grad_compare.py): per tensor
e = max|gpu - r64| / max|r64|, e32 the same for the float32 evaluation, e <= max(4 e32, 2e-6) and e <= 1e-4."""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import rng as orng, torch_ref
from tests import persist_cases as PC

UNSUPPORTED = 'unsupported'
SF_ERR_UNSUPPORTED = 2

# (speaker_follower_amd/csrc/sf_gemm.hip; the line each value mirrors)
LSTM_KS = 4                                   # :983   K-slices of the 16-row kernel
LSTMW_WAVES = 16                              # :1058  K-slices of the 32-row kernel
BWS_WAVES = 8                                 # :1187  K-slices of the fused backward step
FUSED_ROWS, WIDE_ROWS = 16, 32                # :990, :1064
CELL_FUSED_MAX = 1024                         # sf_api.hip: lstm_fwd_i  I + H <= 1024 takes the fused step
BWD_FUSED_MAX_H = 512                         # sf_api_encoder.hip: sf_encoder_lstm_bwd

STEP_FUSED, STEP_WIDE = 'lstm_step_fused_kernel<%d>', 'lstm_step_wide_kernel<%d>'
BWD_FUSED, PW_BWD, PW_FWD = 'lstm_bwd_step_fused_kernel<%d>', 'lstm_pw_bwd_kernel', 'lstm_pw_fwd_kernel<%d>'
PW_FWD_PREFIX = 'lstm_pw_fwd_kernel<'
PERSISTENT = ('enc_persist_kernel', 'enc_bwd_persist_kernel')


def ceil_div(a, b):
    return -(-a // b)


def chunks(H, I=None):
    """total (sf_gemm.hip:2128)."""
    return ceil_div(H, 16) + (ceil_div(I, 16) if I is not None else 0)


def step_kernel(B, H, I=None, ldx=None):
    """lstm_step_fused (sf_gemm.hip:2126-2150): the kernel one recurrent step runs, or UNSUPPORTED."""
    if H % 16 or (I is not None and (I % 4 or (I if ldx is None else ldx) % 4)):
        return UNSUPPORTED
    total = chunks(H, I)
    if B > FUSED_ROWS and H % 8 == 0:
        cw = ceil_div(total, LSTMW_WAVES)
        if cw <= 2:
            return STEP_WIDE % 2
        if cw <= 4:
            return STEP_WIDE % 4
    c = ceil_div(total, LSTM_KS)
    return STEP_FUSED % 8 if c <= 8 else STEP_FUSED % 16 if c <= 16 else UNSUPPORTED


def bwd_step_kernel(H, w_hh_t=True):
    """sf_encoder_lstm_bwd per step (sf_api_encoder.hip) over lstm_bwd_step_fused (sf_gemm.hip:2152-2163)."""
    if not w_hh_t or H % 16 or H > BWD_FUSED_MAX_H:
        return PW_BWD
    c = ceil_div((4 * H) >> 4, BWS_WAVES)
    return BWD_FUSED % 8 if c <= 8 else BWD_FUSED % 16 if c <= 16 else UNSUPPORTED


def cell_kernel(B, I, H, ldx=None):
    """lstm_fwd_i (sf_api.hip): the fused step, or the gate product and `lstm_pw_fwd_kernel<KS>` for some KS."""
    if I + H <= CELL_FUSED_MAX and H % 16 == 0:
        return step_kernel(B, H, I, ldx)
    return PW_FWD_PREFIX


def family_kernels(prof):
    """{name: calls} of the kernels of this family in a _lib.kernel_profile()."""
    return {k: v['calls'] for k, v in prof.rows.items() if k.startswith(('lstm_step_', 'lstm_bwd_step_', 'lstm_pw_'))}


def persistent_kernels(prof):
    return sorted(k for k in prof.rows if k.startswith(PERSISTENT))


# ---------------------------------------------------------------------------------------------- cases
HS = (16, 48, 256, 272, 512, 528, 1024)
Cell = namedtuple('Cell', 'B I H')
CellVariant = namedtuple('CellVariant', 'pad drop_copy p')
Enc = namedtuple('Enc', 'H B')
EncVariant = namedtuple('EncVariant', 'table p gates')
Spk = namedtuple('Spk', 'H B')
Bwd = namedtuple('Bwd', 'H B w_hh_t')
Bi = namedtuple('Bi', 'H B T')
Pw = namedtuple('Pw', 'B I H KS')

CELL_SHAPES = ((256, 256),                    # (I, H): total 32
               (260, 256),                    # total 33, the last chunk 4 of 16 wide
               (768, 256),                    # total 64
               (300, 512),                    # the speaker's cell
               (48, 16), (4, 48))
CELL_BS = (1, 16, 17, 32, 33)
CELL = [Cell(B, I, H) for I, H in CELL_SHAPES for B in CELL_BS]
CELL_VARIANTS = [CellVariant(pad, dc, p) for pad in (0, 4) for dc, p in ((False, 0.0), (True, 0.0), (True, 0.5))]

ENC_HS, ENC_BS, ENC_TS = (16, 512, 528, 1024), (1, 16, 17, 33), (1, 2, 4)
ENCODER = [Enc(H, B) for H in ENC_HS for B in ENC_BS]
ENC_VARIANTS = [EncVariant(True, 0.0, True), EncVariant(True, 0.5, False), EncVariant(False, 0.5, True),
                EncVariant(False, 0.0, False)]
ENC_RAW_STATE = (Enc(528, 17), 2)             # (case, T) of the SF_ENC_RAW_STATE run
ENC_REFUSED_H = 1040                          # total 65: no kernel covers it
ENC_E, ENC_VOCAB = 8, 12

SPEAKER = [Spk(H, B) for H in (512, 1024) for B in (9, 17)]
SPK_TP, SPK_VOCAB = 2, 10
SPK_TEXT_MAX_H = 512                          # sf_attention.hip:663, :1548  the entry's text attention: H <= TXT_CPL * 256

BWD_TS = (1, 2, 4)
BWD_FUSED_CASES = [Bwd(H, B, True) for H in (16, 256, 272, 512) for B in (1, 16, 17)]
BWD_TWO_LAUNCH = [Bwd(528, B, True) for B in (1, 16, 17)] + [Bwd(512, B, False) for B in (1, 16, 17)]
BIDIR = [Bi(256, 1, 3), Bi(256, 17, 3)]

# The slab count KS as observed on the MI355X.  Below 512 rows it is linear_nt's split, min(ceil(2048 / (4H/16 x row
# blocks)), chunks / 4, 8), cut while 4H/64 x KS > 256 once I + H >= 2048: 8, 7 and 4 are what H in HS reaches, KS = 1 is
# not reached from small B.  From 512 rows on the many-row product picks 1 .. 3 slabs by its tile count: the last two cases.
POINTWISE = [Pw(100, 4352, 512, 8),           # the benchmark's gate shape
             Pw(1, 1040, 1024, 4), Pw(3, 2176, 1024, 4), Pw(33, 4352, 1024, 4),
             Pw(17, 2176, 528, 7), Pw(3, 1040, 528, 8),
             Pw(33, 1040, 16, 8), Pw(17, 1040, 272, 8),
             Pw(512, 1040, 48, 2), Pw(1408, 1040, 512, 1)]      # 8 tiles: two slabs; 176 tiles: one

DROP_SEED, DROP_ROW0, SITE = 0x5EED5, 5, 11


def all_kernels():
    """Every kernel name the tables reach (pointwise forward: with the committed KS)."""
    out = set()
    for c in CELL:
        out.add(cell_kernel(c.B, c.I, c.H))
    for c in ENCODER:
        out.add(step_kernel(c.B, c.H))
    for c in SPEAKER:
        out.add(step_kernel(c.B, c.H))
    for c in BWD_FUSED_CASES + BWD_TWO_LAUNCH:
        out.add(bwd_step_kernel(c.H, c.w_hh_t))
    for c in BIDIR:
        out.add(step_kernel(c.B, c.H))
        out.add(bwd_step_kernel(c.H))
    for c in POINTWISE:
        assert cell_kernel(c.B, c.I, c.H) == PW_FWD_PREFIX
        out.add(PW_FWD % c.KS)
    return out


def boundaries():
    """(name, value below, value above, cases on each side) of every edge of the dispatch."""
    tot = [chunks(c.H, c.I) for c in CELL] + [chunks(c.H) for c in ENCODER]
    bs = [c.B for c in CELL + ENCODER]
    bh = [c.H for c in BWD_FUSED_CASES + BWD_TWO_LAUNCH if c.w_hh_t]
    return [('B 16 | 17', 16, 17, bs), ('B 32 | 33', 32, 33, bs), ('total 32 | 33', 32, 33, tot),
            ('total 64 | 65', 64, 65, tot + [chunks(ENC_REFUSED_H)]), ('H 256 | 272', 256, 272, bh),
            ('H 512 | 528', 512, 528, bh)]


# ---------------------------------------------------------------------------------------- exact family
_A, _C = 35, 11                               # odd, coprime to every 4H and H of HS


def _mix(n):
    """A fixed 0/1 pattern over row indices (the top bit of a Fibonacci hash)."""
    return ((np.asarray(n, np.int64) * 2654435761) >> 31) & 1


def exact_runs(H, I=None):
    """Runs of a case: two (the columns held at zero alternate) for each 4H-row window over the K columns."""
    return 2 * ceil_div((I or 0) + H, 4 * H)


def exact_selection(H, I, run):
    """col [4H]: the operand column (of [x | h0]) row n = gate H + unit weighs, an asymmetric function of (gate, unit);
    sign [4H]: -1 on some rows of gate g, +1 elsewhere; held [K]: columns held at zero in this run."""
    K = (I or 0) + H
    n = np.arange(4 * H)
    gate, unit = n // H, n % H
    pi = ((4 * unit + gate) * _A + _C) % (4 * H)
    col = (pi + (run // 2) * 4 * H) % K
    sign = np.where((gate == 2) & (unit % 3 == 1), -1.0, 1.0)
    held = ((np.arange(K) >> 2) & 1) == (run % 2)
    return col, sign, held


def exact_cell(B, H, I=None, run=0, vocab=None, seed=0):
    """One step of the exact family: dict(x [B, I] or None, h0, c0, w_ih, w_hh, b_ih, b_hh, table [vocab, 4H] / tok [B] or
    None), float32.  Rows whose column is held draw their pre-activation from b_ih, b_hh or the table instead."""
    rng = np.random.default_rng([seed, B, H, I or 0, run, 59])
    I0 = I or 0
    K = I0 + H
    col, sign, held = exact_selection(H, I, run)
    n = np.arange(4 * H)
    W = np.zeros((4 * H, K), np.float32)
    W[n, col] = sign
    a = (40.0 * rng.integers(0, 2, size=(B, K))).astype(np.float32)
    a[:, held] = 0
    side = held[col]                                        # rows fed from a bias / the table
    kind = n % (3 if vocab else 2)
    amp = (40.0 * sign * _mix(n)).astype(np.float32)
    d = dict(x=np.ascontiguousarray(a[:, :I0]) if I else None, h0=np.ascontiguousarray(a[:, I0:]),
             c0=(64.0 * rng.integers(-1, 2, size=(B, H))).astype(np.float32),
             w_ih=np.ascontiguousarray(W[:, :I0]) if I else None, w_hh=np.ascontiguousarray(W[:, I0:]),
             b_ih=np.where(side & (kind == 0), amp, 0).astype(np.float32),
             b_hh=np.where(side & (kind == 1), amp, 0).astype(np.float32), table=None, tok=None)
    if vocab:
        t = 40.0 * sign[None, :] * rng.integers(0, 2, size=(vocab, 4 * H))
        d['table'] = np.where((side & (kind == 2))[None, :], t, 0).astype(np.float32)
        d['tok'] = rng.integers(0, vocab, size=B).astype(np.int64)
    return d


def exact_columns_covered(H, I=None, vocab=None):
    """Over the runs of a case: does every operand column carry a weight in a run in which it carries data?"""
    K = (I or 0) + H
    seen = np.zeros(K, bool)
    for run in range(exact_runs(H, I)):
        col, _, held = exact_selection(H, I, run)
        seen[col[~held[col]]] = True
    return bool(seen.all())


def cell_np(d, dtype=np.float64, drop_chunk=None, swap_gates=None):
    """The cell on the dict of exact_cell / dense_cell, every operation in `dtype`: gates [B, 4H] (activated), c1, h1 and
    `exact` (where h1 is exact in the exact family).  Two planted errors for the host test: drop_chunk = the 16-wide chunk
    of the reduction (h0's chunks first, then x's: the kernels' order) left out; swap_gates = (g1, g2) swapped in the
    first 16 x 16 tile."""
    f = lambda a: np.asarray(a, dtype)                     # noqa: E731
    B, H = d['h0'].shape
    pre = np.zeros((B, 4 * H), dtype) + f(d['b_ih']) + f(d['b_hh'])
    if d.get('table') is not None:
        pre = pre + f(d['table'])[d['tok']]
    c = 0
    for a, w in ((d['h0'], d['w_hh']), (d.get('x'), d.get('w_ih'))):
        if a is None:
            continue
        a = f(a).copy()
        nc = ceil_div(a.shape[1], 16)
        if drop_chunk is not None and c <= drop_chunk < c + nc:
            a[:, 16 * (drop_chunk - c):16 * (drop_chunk - c + 1)] = 0
        c += nc
        pre = pre + a @ f(w).T
    if swap_gates:
        g1, g2 = swap_gates
        t = pre[:16, g1 * H:g1 * H + 16].copy()
        pre[:16, g1 * H:g1 * H + 16] = pre[:16, g2 * H:g2 * H + 16]
        pre[:16, g2 * H:g2 * H + 16] = t
    one = dtype(1)
    sig = lambda v: one / (one + np.exp(-v))               # noqa: E731
    with np.errstate(over='ignore'):                       # (peaky, float32: exp overflows to inf, the gate is 0)
        ig, fg, gg, og = sig(pre[:, :H]), sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
    c1 = fg * f(d['c0']) + ig * gg
    h1 = og * np.tanh(c1)
    return dict(gates=np.concatenate((ig, fg, gg, og), 1), c1=c1, h1=h1, exact=(c1 == 0) | (np.abs(c1) >= 16))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def same_bits(got, want, where=None):
    """float32 arrays equal bit for bit (np.array_equal on the int32 view), optionally only `where`."""
    g, w = bits(got), bits(want)
    if g.shape != w.shape:
        return False
    return bool(np.array_equal(g, w) if where is None else np.array_equal(g[where], w[where]))


def libm_facts(exp, tanh):
    """The four facts the exact family rests on, for float32 `exp` / `tanh`: a list of the ones that do NOT hold."""
    f = np.float32
    bad = []
    if exp(f(0)) != f(1):
        bad.append('expf(0) != 1')
    if not exp(f(-40)) < f(2.0 ** -25):
        bad.append('expf(-40) >= 2^-25')
    if tanh(f(0)) != f(0):
        bad.append('tanhf(0) != 0')
    for v in (16, 31, 32, 33, 63.5, 64, 65):
        if tanh(f(v)) != f(1) or tanh(f(-v)) != f(-1):
            bad.append('tanhf(+-%g) != +-1' % v)
    return bad


# ---------------------------------------------------------------------------------------- dense family
def dense_cell(B, H, I=None, peaky=False, vocab=None, seed=0):
    """N(0, 1) operands, weights and biases x H^-0.5 (peaky: x 8), the table N(0, 1) x (peaky: 2)."""
    rng = np.random.default_rng([seed, B, H, I or 0, int(peaky), 61])
    k = H ** -0.5 * (8.0 if peaky else 1.0)
    r = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)          # noqa: E731
    d = dict(x=r(B, I) if I else None, h0=r(B, H), c0=r(B, H), w_ih=r(4 * H, I, scale=k) if I else None,
             w_hh=r(4 * H, H, scale=k), b_ih=r(4 * H, scale=k), b_hh=r(4 * H, scale=k), table=None, tok=None)
    if vocab:
        d['table'] = r(vocab, 4 * H, scale=2.0 if peaky else 1.0)
        d['tok'] = rng.integers(0, vocab, size=B).astype(np.int64)
    return d


def cell_reference(d, dtype):
    """float64 numpy {gates, c1, h1} of the cell evaluated in the torch `dtype`; with an input segment h1 and c1 are
    oracle/torch_ref.lstm_cell's."""
    out = {k: np.asarray(v, np.float64) for k, v in cell_np(d, np.float64 if dtype == torch.float64 else np.float32).items()}
    if d.get('x') is not None and d.get('table') is None:
        t = lambda a: torch.as_tensor(a).to(dtype)         # noqa: E731
        h1, c1 = torch_ref.lstm_cell(t(d['x']), t(d['h0']), t(d['c0']), t(d['w_ih']), t(d['w_hh']), t(d['b_ih']), t(d['b_hh']))
        out['h1'], out['c1'] = h1.double().numpy(), c1.double().numpy()
    return out


def cell_backward_reference(d, dh1, dc1, dtype):
    """Autograd of oracle/torch_ref.lstm_cell in `dtype` under sum(h1 dh1) + sum(c1 dc1): float64 numpy dx, dh0, dc0 and
    the four weight gradients."""
    t = lambda a, g=True: torch.as_tensor(a).to(dtype).requires_grad_(g)       # noqa: E731
    x, h, c = t(d['x']), t(d['h0']), t(d['c0'])
    w = [t(d[k]) for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')]
    h1, c1 = torch_ref.lstm_cell(x, h, c, *w)
    ((h1 * t(dh1, False)).sum() + (c1 * t(dc1, False)).sum()).backward()
    n = lambda v: v.grad.double().numpy()                  # noqa: E731
    return dict(dx=n(x), dh0=n(h), dc0=n(c), w_ih=n(w[0]), w_hh=n(w[1]), b_ih=n(w[2]), b_hh=n(w[3]))


@functools.lru_cache(maxsize=8)
def encoder_weights(H, family='plain', bidir=False, seed=0):
    """An EncoderLSTM state (numpy, keyed like its state_dict; E = ENC_E, vocab = ENC_VOCAB; bidir: H per direction).
    family 'plain' / 'peaky': N(0, 1) x H^-0.5 (x 8); 'lattice': the exact family's step 0 -- one weight +-1 per row of
    W_hh, the embedding on {0, 40}, and each gate row fed by exactly one of b_ih, b_hh or one embedding column, on
    {0, +-40} with the minus sign on gate g only."""
    rng = np.random.default_rng([seed, H, int(bidir), ('plain', 'peaky', 'lattice').index(family), 67])
    r = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)          # noqa: E731
    E, V, nd = ENC_E, ENC_VOCAB, 2 if bidir else 1
    k = H ** -0.5 * (8.0 if family == 'peaky' else 1.0)
    w = {'embedding.weight': r(V, E), 'encoder2decoder.weight': r(nd * H, nd * H, scale=(nd * H) ** -0.5),
         'encoder2decoder.bias': r(nd * H, scale=(nd * H) ** -0.5)}
    if family == 'lattice':
        w['embedding.weight'] = (40.0 * rng.integers(0, 2, size=(V, E))).astype(np.float32)
    for sfx in ('', '_reverse')[:nd]:
        if family != 'lattice':
            w.update({'lstm.weight_ih_l0' + sfx: r(4 * H, E, scale=k), 'lstm.weight_hh_l0' + sfx: r(4 * H, H, scale=k),
                      'lstm.bias_ih_l0' + sfx: r(4 * H, scale=k), 'lstm.bias_hh_l0' + sfx: r(4 * H, scale=k)})
            continue
        col, sign, _ = exact_selection(H, None, 0)
        n = np.arange(4 * H)
        kind = n % 3
        amp = (40.0 * sign * _mix(n)).astype(np.float32)
        w_hh = np.zeros((4 * H, H), np.float32)
        w_hh[n, col] = sign
        w_ih = np.zeros((4 * H, E), np.float32)
        w_ih[n[kind == 2], (n[kind == 2] // 3) % E] = sign[kind == 2]
        w.update({'lstm.weight_ih_l0' + sfx: w_ih, 'lstm.weight_hh_l0' + sfx: w_hh,
                  'lstm.bias_ih_l0' + sfx: np.where(kind == 0, amp, 0).astype(np.float32),
                  'lstm.bias_hh_l0' + sfx: np.where(kind == 1, amp, 0).astype(np.float32)})
    return w


def xw_table(w, sfx=''):
    """[vocab, 4H] = embedding W_ih^T, formed in float64 (the lattice family's rows hold one term each: exact)."""
    return (w['embedding.weight'].astype(np.float64) @ w['lstm.weight_ih_l0' + sfx].astype(np.float64).T).astype(np.float32)


def ctx_mask(p, B, T, width):
    """The ctx dropout mask [B, T, width] of site SITE (None: dropout off)."""
    if not p:
        return None
    return orng.dropout_mask(DROP_SEED, SITE, DROP_ROW0 + np.arange(B), T * width, p).reshape(B, T, width)


ENC_KEYS = ('ctx', 'h', 'c', 'gates', 'hs', 'cs')


def encoder_reference(w, seq, lens, mask, dtype, raw_state=False, advance_row=None):
    """PC.encoder_model as float64 numpy {ctx, h, c, gates, hs, cs} (raw_state: h = the raw h_T).  advance_row: that row
    runs one step longer than its length (a planted error for the host test)."""
    lens = list(lens)
    if advance_row is not None:
        lens[advance_row] += 1
    m = PC.encoder_model(w, seq, lens, mask, dtype)
    n = lambda t: t.detach().double().numpy()              # noqa: E731
    f = m['f']
    return dict(ctx=n(m['ctx']), h=n(f['h'] if raw_state else m['decoder_init']), c=n(m['c_t']), gates=n(f['gates']),
                hs=n(f['hs']), cs=n(f['cs']))


# -------------------------------------------------------------------------------- exact backward tapes
def exact_backward(B, T, H, lens, seed=0):
    """Hand-made tapes of T steps: gates [T, B, 4H] dyadic (i on {1/2, 1/4}, f on {1/2, 3/4}, g on {0, +-1/2}, o on
    {1/2, 3/4}), cs [T + 1, B, H] on {0, +-32}, dctx [B, T, H] and d_ct [B, H] small integers (dctx also beyond the
    lengths), W_hh [4H, H] whose transpose holds one 1 per row: dh[b, j] = dgates[b, sel(j)]."""
    rng = np.random.default_rng([seed, B, T, H, 71])
    pick = lambda vals, *s: rng.choice(np.asarray(vals, np.float32), size=s)       # noqa: E731
    gates = np.concatenate((pick((0.5, 0.25), T, B, H), pick((0.5, 0.75), T, B, H), pick((0.0, 0.5, -0.5), T, B, H),
                            pick((0.5, 0.75), T, B, H)), 2)
    cs = pick((0.0, 0.0, 32.0, -32.0), T + 1, B, H)
    j = np.arange(H)
    sel = (j % 4) * H + (j * _A + _C) % H
    w_hh = np.zeros((4 * H, H), np.float32)
    w_hh[sel, j] = 1
    return dict(gates=gates, cs=cs, w_hh=w_hh, lens=list(lens), dctx=rng.integers(-3, 4, size=(B, T, H)).astype(np.float32),
                d_ct=rng.integers(-2, 3, size=(B, H)).astype(np.float32))


def backward_np(tp, mask=None, dtype=np.float64, d_h=None, leak_dctx=False):
    """The backward recurrence on tapes (dict of exact_backward, or gates / cs / w_hh / lens / dctx / d_ct of a dense run):
    dgates [T, B, 4H] in `dtype`.  mask: the ctx dropout mask [B, T, H].  leak_dctx: dctx beyond a length is added too
    (the planted error)."""
    f = lambda a: np.asarray(a, dtype)                     # noqa: E731
    gates, cs, w_hh = f(tp['gates']), f(tp['cs']), f(tp['w_hh'])
    T, B, H = gates.shape[0], gates.shape[1], cs.shape[2]
    lens = np.asarray(tp['lens'])
    dctx = f(tp['dctx']) * (f(mask) if mask is not None else dtype(1))
    dh = f(d_h) if d_h is not None else np.zeros((B, H), dtype)
    dc = f(tp['d_ct'])
    one = dtype(1)
    out = np.zeros((T, B, 4 * H), dtype)
    for t in range(T - 1, -1, -1):
        dead = (t >= lens)[:, None]
        dh = dh + (dctx[:, t] if leak_dctx else np.where(dead, dtype(0), dctx[:, t]))
        ig, fg, gg, og = (gates[t][:, g * H:(g + 1) * H] for g in range(4))
        c0, tc = cs[t], np.tanh(cs[t + 1])
        dout = dh * tc
        dcl = dc + dh * og * (one - tc * tc)
        dg = np.concatenate((dcl * gg * ig * (one - ig), dcl * c0 * fg * (one - fg), dcl * ig * (one - gg * gg),
                             dout * og * (one - og)), 1)
        dg = np.where(dead, dtype(0), dg)
        dc = np.where(dead, dc, dcl * fg)
        dh = np.where(dead, dh, dtype(0)) + dg @ w_hh
        out[t] = dg
    return out


def exact_cell_backward(B, H, I, seed=0):
    """One cell backward on hand-made tapes (exact_backward's value sets) with one 1 per column of W_ih and W_hh:
    dx[b, i] = dgates[b, sel_x(i)], dh0[b, j] = dgates[b, sel_h(j)].  Returns (inputs, expected dx / dh0 / dc0)."""
    tp = exact_backward(B, 1, H, [1] * B, seed)
    rng = np.random.default_rng([seed, B, H, I, 73])
    i = np.arange(I)
    sel_x = ((i % 4) * H + (i * _A + _C) % H + (i // (4 * H)) * 7) % (4 * H)
    w_ih = np.zeros((4 * H, I), np.float32)
    w_ih[sel_x, i] = 1
    dh1 = rng.integers(-3, 4, size=(B, H)).astype(np.float32)
    d = dict(gates=tp['gates'][0], c0=tp['cs'][0], c1=tp['cs'][1], w_ih=w_ih, w_hh=tp['w_hh'], dh1=dh1, dc1=tp['d_ct'],
             x=(40.0 * rng.integers(0, 2, size=(B, I))).astype(np.float32), h0=np.zeros((B, H), np.float32))
    out = {}
    for dtype in (np.float32, np.float64):
        one = dict(tp, dctx=dh1[:, None, :])
        dg = backward_np(one, dtype=dtype)[0]
        fg = np.asarray(d['gates'][:, H:2 * H], dtype)
        tc = np.tanh(np.asarray(d['c1'], dtype))
        dcl = np.asarray(d['dc1'], dtype) + np.asarray(dh1, dtype) * np.asarray(d['gates'][:, 3 * H:], dtype) * (dtype(1) - tc * tc)
        out[dtype] = dict(dx=dg @ np.asarray(w_ih, dtype), dh0=dg @ np.asarray(d['w_hh'], dtype), dc0=dcl * fg)
    return d, out[np.float32], out[np.float64]


# ------------------------------------------------------------------------------------------ comparing
def compare(what, got, r64, r32, keys, rows=None):
    """PC.compare under the tag of this family: every (e, e32) is printed and appended to `rows`."""
    PC.compare(what, got, r64, r32, keys, rows=rows)


def padded(a, pad, tail_rows=2):
    """`a` [B, N] in rows of stride N + pad, NaN in the padding columns and in `tail_rows` rows behind the last."""
    B, N = a.shape
    out = np.full((B + tail_rows, N + pad), np.nan, np.float32)
    out[:B, :N] = a
    return out
