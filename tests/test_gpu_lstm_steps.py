"""The per-step LSTM kernels -- lstm_step_fused_kernel<8|16>, lstm_step_wide_kernel<2|4>, lstm_bwd_step_fused_kernel<8|16>
(csrc/sf_gemm.hip), lstm_pw_fwd_kernel<KS>, lstm_pw_bwd_kernel (csrc/sf_pointwise.hip, csrc/sf_lstm_pw.h) -- one launch at
a time through the C entries, at every edge of their dispatch (tests/lstm_step_cases.py: the mirror of the dispatch, the
tables, the two input families and the models; tests/test_lstm_step_cases_host.py checks those on the host and shows that
the comparators refuse a swapped gate, a dropped chunk, shifted rows, an advanced dead row and a leaked dctx).

Every case runs under _lib.kernel_profile(): the kernel the mirror names must have run, once per step, and no other
kernel of the family; on the per-step encoder cases neither enc_persist_kernel nor enc_bwd_persist_kernel.  Inputs with a
row stride carry NaN in their padding columns and in two rows behind the last; every output is NaN-filled with guard rows
behind it (and padding columns where it has a stride) that must come back untouched.  Every launch is issued twice and
must give the same bits.

EXACT family: gates, c1 and h1 (where c1 == 0 or |c1| >= 16) bit for bit against the float32 model, which the host test
shows equal to the float64 one there; the backward's dgates / dx / dh0 / dc0 on hand-made tapes bit for bit.  The encoder
entry starts from the zero state it fills itself, so only its step 0 is on the lattice (family 'lattice': step 0 bit for
bit, everything under the dense rule as well).  In both families, bit for bit: dead rows (h1 == h0, c1 == c0, ctx +0.0;
backward: dgates == 0), and the dropped copies -- ctx and cat2[:, H:] equal the launch's own h1 times the mask of
oracle/rng.py (p = 0.5, scale 2).
DENSE family: per tensor e = max|gpu - r64| / max|r64| against e32 of the float32 evaluation of the same model,
e <= max(4 e32, 2e-6) and e <= 1e-4 (tests/grad_compare.py; no case has a bound of its own).

Measured on an MI355X: per kernel the comparison that used the largest share of its bound, as (e, e32).  `-s` prints
every figure (under the comparator's tag, `[persist]`) and, at the end of the module, this table:
    lstm_step_fused_kernel<8>        gates   (5.1e-06, 2.1e-06)  0.62 of the bound   B 1, I 256, H 256, peaky
    lstm_step_fused_kernel<16>       h1      (2.1e-06, 7.5e-07)  0.69                B 1, I 260, H 256, peaky
    lstm_step_wide_kernel<2>         h1      (1.0e-06, 6.0e-07)  0.42                B 33, I 4, H 48, peaky
    lstm_step_wide_kernel<4>         h       (4.8e-07, 5.0e-07)  0.24                H 1024, B 33, T 2, lattice
    lstm_bwd_step_fused_kernel<8>    dgates  (5.8e-07, 3.3e-07)  0.29                H 16, B 16, T 4, peaky
    lstm_bwd_step_fused_kernel<16>   dgates  (2.1e-06, 1.8e-06)  0.29                H 512, B 1, T 4, peaky
    lstm_pw_bwd_kernel               dx      (5.2e-06, 2.6e-06)  0.49                B 17, I 2176, H 528, peaky
    lstm_pw_fwd_kernel<1>            h1      (1.1e-06, 1.4e-06)  0.19                B 1408, I 1040, H 512
    lstm_pw_fwd_kernel<2>            h1      (2.6e-06, 2.8e-06)  0.23                B 512, I 1040, H 48
    lstm_pw_fwd_kernel<4>            h1      (6.6e-06, 3.0e-06)  0.55                B 1, I 1040, H 1024, peaky
    lstm_pw_fwd_kernel<7>            c1      (3.4e-06, 2.1e-06)  0.41                B 17, I 2176, H 528, peaky
    lstm_pw_fwd_kernel<8>            c1      (1.9e-06, 1.5e-06)  0.32                B 3, I 1040, H 528, peaky
    bidirectional, per step          every tensor of both directions within (2.0e-07, 2.5e-07)
    weight gradients                 the largest share 0.64: w_hh (1.0e-05, 4.1e-06) behind lstm_pw_bwd_kernel at
                                     B 17, I 2176, H 528, peaky
Every exact comparison held bit for bit: the device's expf and tanhf return 1, < 2^-25, 0 and +-1 at the four arguments
the family rests on.  No case has a bound of its own.

The slab count KS as observed (B, I, H -> KS): (100, 4352, 512) 8, the benchmark's gate shape; (1, 1040, 1024),
(3, 2176, 1024), (33, 4352, 1024) 4; (17, 2176, 528) 7; (3, 1040, 528), (33, 1040, 16), (17, 1040, 272) 8.  KS = 1 is not
reached from B <= 100 at any H of the table: below 512 rows the split is at least 4 there.  It takes the many-row product,
which picks 1 .. 3 slabs by its tile count: (512, 1040, 48) gives 2 and (1408, 1040, 512) gives 1; those two cases are
the only ones above B = 100.

Found: no kernel of the family was wrong.  Two limits of the entries around them were not written down:
  * sf_encoder_lstm_fwd with SF_ENC_PER_STEP returns SF_ERR_UNSUPPORTED above H = 1024 (65 chunks at H = 1040), after
    it has embedded the tokens and filled the zero state; include/sf_hip.h now says so, and
    test_encoder_per_step_refuses_more_than_64_chunks pins it.  model.EncoderLSTM has no fallback for that status.
  * sf_speaker_decoder_fwd takes its lookup step for H <= 1024, but the text attention behind it covers H <= 512: at
    H = 1024 the step runs and the entry then returns SF_ERR_UNSUPPORTED.  test_speaker_decoder_lookup_step pins that and
    compares the step's outputs all the same.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rng as orng                                        # noqa: E402
from tests import grad_compare as GC                                  # noqa: E402
from tests import lstm_step_cases as LC                               # noqa: E402
from tests import persist_cases as PC                                 # noqa: E402
from tests.test_gpu_persistent_edges import Guarded, dev, reference_grads        # noqa: E402

ROWS = []                                   # (what, tensor, e, e32, bound) of every comparison of the session
E, V = LC.ENC_E, LC.ENC_VOCAB
F32 = np.float32


def _api():
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import ptr, ws_args, dropout_arg
    return _lib, ptr, ws_args, dropout_arg


def drop_arg(p):
    return _api()[3](p, LC.DROP_SEED, LC.DROP_ROW0)


def addr(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * offset)


def profiled(fn):
    """fn() under the kernel profile, synchronised: (its result, {family kernel: calls}, persistent kernels)."""
    _lib = _api()[0]
    with _lib.kernel_profile() as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, LC.family_kernels(prof), LC.persistent_kernels(prof)


def untouched(g, skip=()):
    for k, v in g.items():
        if v is not None and k not in skip:
            assert v.untouched(), 'guard rows of %s were written' % k


def same_twice(a, b, keys):
    for k in keys:
        if a.get(k) is not None:
            assert np.array_equal(LC.bits(a[k]), LC.bits(b[k])), 'the same launch twice: %s differs' % k


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    worst = {}
    for what, key, e, e32, b in ROWS:
        kern = what.split()[0]
        if kern not in worst or e / b > worst[kern][0]:
            worst[kern] = (e / b, what, key, e, e32)
    for kern in sorted(worst):
        _, what, key, e, e32 = worst[kern]
        print('[lstm-steps] worst of %-34s %-12s (e, e32) = (%.1e, %.1e)  share of bound %.2f  [%s]'
              % (kern, key, e, e32, worst[kern][0], what))


# ------------------------------------------------------------------------- the cell with an input segment
def lstm_w(wd, transposed=False):
    _lib = _api()[0]
    t = (lambda k: addr(wd[k + '_t'])) if transposed else (lambda k: None)
    return _lib.LstmW(addr(wd['w_ih']), addr(wd['w_hh']), addr(wd['b_ih']), addr(wd['b_hh']), t('w_ih'), t('w_hh'))


def cell_device(d):
    return {k: dev(d[k]) for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh', 'h0', 'c0')}


def cell_fwd(d, wd, case, v):
    """sf_lstm_cell_fwd on guarded buffers: (outputs, buffers, family kernels)."""
    _lib, ptr, ws_args, _ = _api()
    B, I, H = case.B, case.I, case.H
    x = dev(LC.padded(d['x'], v.pad))
    h0, c0 = dev(LC.padded(d['h0'], 0)), dev(LC.padded(d['c0'], 0))
    g = dict(h1=Guarded(B, H), c1=Guarded(B, H), gates=Guarded(B, 4 * H), cat2=Guarded(B, 2 * H) if v.drop_copy else None)
    lw = lstm_w(wd)
    _, fam, _ = profiled(lambda: _lib.call(
        'sf_lstm_cell_fwd', C.byref(lw), B, I, H, ptr(x), I + v.pad, ptr(h0), ptr(c0), g['h1'].ptr(), g['c1'].ptr(),
        g['gates'].ptr(), addr(g['cat2'].full, H) if v.drop_copy else None, 2 * H, drop_arg(v.p), LC.SITE,
        *ws_args(x.device)))
    untouched(g)
    return {k: b.np() for k, b in g.items() if b is not None}, g, fam


def dropped(h, mask):
    """h times the mask as the kernels form it: +0.0 where the element is dropped."""
    return np.where(mask != 0, h * mask, F32(0)).astype(F32)


def check_dropped_copy(cat2, h1, p, stream, H):
    """cat2 [B, 2H]: the first half still the sentinel, the second the launch's own h1 times the mirror's mask."""
    B = h1.shape[0]
    assert np.isnan(cat2[:, :H]).all(), 'the columns in front of the dropped copy were written'
    mask = orng.dropout_mask(LC.DROP_SEED, stream, LC.DROP_ROW0 + np.arange(B), H, p)
    assert LC.same_bits(cat2[:, H:], dropped(h1, mask)), 'the dropped copy is not h1 times the mirror\'s mask'
    if p:
        assert 0.3 < (mask == 0).mean() < 0.7


def check_cell(what, out, d, family, r64, r32):
    for k in ('gates', 'c1', 'h1'):
        assert np.isfinite(out[k]).all(), '%s: %s holds non-finite values' % (what, k)
    if family == 'exact':
        m = LC.cell_np(d, F32)
        assert LC.same_bits(out['gates'], m['gates']), '%s: gates differ from the exact model' % what
        assert LC.same_bits(out['c1'], m['c1']), '%s: c1 differs from the exact model' % what
        assert LC.same_bits(out['h1'], m['h1'], m['exact']), '%s: h1 differs from the exact model where it is exact' % what
    LC.compare(what, out, r64, r32, ('gates', 'c1', 'h1'), rows=ROWS)


def families(H, I):
    """(family, run) pairs of a cell shape."""
    return [('exact', r) for r in range(LC.exact_runs(H, I))] + [('plain', 0), ('peaky', 0)]


def cell_inputs(family, run, B, H, I, vocab=None):
    if family == 'exact':
        return LC.exact_cell(B, H, I, run, vocab)
    return LC.dense_cell(B, H, I, family == 'peaky', vocab)


@pytest.mark.parametrize('case', LC.CELL, ids=lambda c: 'B%d-I%d-H%d' % c)
def test_cell_step_with_an_input_segment(case):
    """sf_lstm_cell_fwd at I + H <= 1024: one fused step over [h0 | x], both row-tile kernels, both chunk counts."""
    kernel = LC.cell_kernel(case.B, case.I, case.H)
    for family, run in families(case.H, case.I):
        d = cell_inputs(family, run, case.B, case.H, case.I)
        wd = cell_device(d)
        r64, r32 = LC.cell_reference(d, torch.float64), LC.cell_reference(d, torch.float32)
        first = None
        for v in LC.CELL_VARIANTS:
            what = '%s B%d I%d H%d %s%d ldx+%d%s' % (kernel, case.B, case.I, case.H, family, run, v.pad,
                                                      ' drop%.1f' % v.p if v.drop_copy else '')
            out, g, fam = cell_fwd(d, wd, case, v)
            assert fam == {kernel: 1}, (what, fam)
            if first is None:
                check_cell(what, out, d, family, r64, r32)
                first = out
                again, _, _ = cell_fwd(d, wd, case, v)
                same_twice(out, again, ('gates', 'c1', 'h1'))
            else:
                same_twice(out, first, ('gates', 'c1', 'h1'))          # neither the stride nor the copy changes a bit
            if v.drop_copy:
                check_dropped_copy(out['cat2'], out['h1'], v.p, LC.SITE, case.H)


# ------------------------------------------------------------------ the gate product and its pointwise kernels
@pytest.mark.parametrize('case', LC.POINTWISE, ids=lambda c: 'B%d-I%d-H%d-KS%d' % c)
def test_pointwise_forward_adds_the_slabs_of_the_gate_product(case):
    """sf_lstm_cell_fwd at I + H > 1024: lstm_pw_fwd_kernel<KS> with the KS observed on the MI355X (LC.POINTWISE)."""
    kernel = LC.PW_FWD % case.KS
    cell = LC.Cell(case.B, case.I, case.H)
    fams = families(case.H, case.I) if case.B <= 100 else [('exact', 0), ('exact', 1), ('plain', 0)]
    for family, run in fams:
        d = cell_inputs(family, run, case.B, case.H, case.I)
        wd = cell_device(d)
        r64, r32 = LC.cell_reference(d, torch.float64), LC.cell_reference(d, torch.float32)
        first = None
        for v in (LC.CellVariant(0, False, 0.0), LC.CellVariant(4, True, 0.5)):
            what = '%s B%d I%d H%d %s%d ldx+%d' % (kernel, case.B, case.I, case.H, family, run, v.pad)
            out, g, fam = cell_fwd(d, wd, cell, v)
            assert fam == {kernel: 1}, (what, fam)
            if first is None:
                check_cell(what, out, d, family, r64, r32)
                first = out
            else:
                same_twice(out, first, ('gates', 'c1', 'h1'))
                check_dropped_copy(out['cat2'], out['h1'], v.p, LC.SITE, case.H)


def cell_bwd(d, wd, B, I, H, tapes, dh1, dc1, pad, transposed, grads):
    """sf_lstm_cell_bwd on guarded buffers: (outputs, family kernels)."""
    _lib, ptr, ws_args, _ = _api()
    x = dev(LC.padded(d['x'], pad))
    ins = {k: dev(LC.padded(a, 0)) for k, a in dict(h0=d['h0'], c0=d['c0'], c1=tapes['c1'], gates=tapes['gates'], dh1=dh1,
                                                    dc1=dc1).items()}
    g = dict(dx=Guarded(B, I + pad), dh0=Guarded(B, H), dc0=Guarded(B, H))
    gw = {k: torch.zeros_like(wd[k]) for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')} if grads else None
    lw = lstm_w(wd, transposed)
    lg = lstm_w(gw) if grads else None
    _, fam, _ = profiled(lambda: _lib.call(
        'sf_lstm_cell_bwd', C.byref(lw), C.byref(lg) if grads else None, B, I, H, ptr(x), I + pad, ptr(ins['h0']),
        ptr(ins['c0']), ptr(ins['c1']), ptr(ins['gates']), ptr(ins['dh1']), ptr(ins['dc1']), g['dx'].ptr(), I + pad,
        g['dh0'].ptr(), g['dc0'].ptr(), *ws_args(x.device)))
    untouched(g)
    out = {k: b.np() for k, b in g.items()}
    assert np.isnan(out['dx'][:, I:]).all(), 'the padding columns of dx were written'
    out['dx'] = out['dx'][:, :I]
    if grads:
        out.update({k: t.cpu().numpy() for k, t in gw.items()})
    return out, fam


CELL_BWD = [(3, 48, 16), (17, 4, 48), (33, 300, 512), (100, 4352, 512), (17, 2176, 528)]


@pytest.mark.parametrize('B,I,H', CELL_BWD, ids=lambda v: str(v))
def test_cell_backward_through_the_pointwise_kernel(B, I, H):
    """sf_lstm_cell_bwd: lstm_pw_bwd_kernel and the products behind it, on hand-made exact tapes (dx, dh0, dc0 bit for
    bit) and on the tapes of a dense forward against float64 autograd."""
    d, r32, r64 = LC.exact_cell_backward(B, H, I)
    wd = {k: dev(d[k]) for k in ('w_ih', 'w_hh')}
    wd.update(b_ih=None, b_hh=None, w_ih_t=wd['w_ih'].t().contiguous(), w_hh_t=wd['w_hh'].t().contiguous())
    for transposed in (False, True):
        out, fam = cell_bwd(d, wd, B, I, H, d, d['dh1'], d['dc1'], 4, transposed, False)
        assert fam == {LC.PW_BWD: 1}, fam
        for k in ('dx', 'dh0', 'dc0'):
            assert LC.same_bits(out[k], r32[k]), 'exact backward (transposed weights: %s): %s differs' % (transposed, k)
    rng = np.random.default_rng([B, I, H, 79])
    for peaky in (False, True):
        d = LC.dense_cell(B, H, I, peaky)
        wd = cell_device(d)
        wd.update(w_ih_t=wd['w_ih'].t().contiguous(), w_hh_t=wd['w_hh'].t().contiguous())
        tapes, _, _ = cell_fwd(d, wd, LC.Cell(B, I, H), LC.CellVariant(0, False, 0.0))
        dh1, dc1 = (rng.standard_normal((B, H)).astype(F32) for _ in range(2))
        g64, g32 = LC.cell_backward_reference(d, dh1, dc1, torch.float64), LC.cell_backward_reference(d, dh1, dc1, torch.float32)
        what = '%s B%d I%d H%d %s' % (LC.PW_BWD, B, I, H, 'peaky' if peaky else 'plain')
        out, fam = cell_bwd(d, wd, B, I, H, tapes, dh1, dc1, 4, True, True)
        assert fam == {LC.PW_BWD: 1}, fam
        LC.compare(what, out, g64, g32, ('dx', 'dh0', 'dc0'), rows=ROWS)
        names = ('w_ih', 'w_hh', 'b_ih', 'b_hh')
        GC.compare_grads({k: out[k] for k in names}, {k: g64[k] for k in names}, g32, what=what,
                         blocks=dict(w_ih=GC.lstm_blocks(4 * H, cols=I), w_hh=GC.lstm_blocks(4 * H, cols=H),
                                     b_ih=GC.lstm_blocks(4 * H), b_hh=GC.lstm_blocks(4 * H)))
        again, _ = cell_bwd(d, wd, B, I, H, tapes, dh1, dc1, 4, True, True)
        same_twice(out, again, ('dx', 'dh0', 'dc0'))


# ------------------------------------------------------------------------------ the encoder, per step
@functools.lru_cache(maxsize=3)
def encoder_device(H, family, bidir=False):
    """(state as numpy, the same on the device with the tables and W_hh^T of each direction)."""
    w = LC.encoder_weights(H, family, bidir)
    wd = {k: dev(v) for k, v in w.items()}
    for sfx in ('', '_reverse')[:2 if bidir else 1]:
        wd['table' + sfx] = dev(LC.xw_table(w, sfx))
        wd['w_hh_t' + sfx] = wd['lstm.weight_hh_l0' + sfx].t().contiguous()
    return w, wd


def encoder_w(wd, table=True, w_hh_t=True, flags=0, sfx='', e2d=True):
    _lib = _api()[0]
    lw = _lib.LstmW(*(addr(wd['lstm.%s_l0%s' % (n, sfx)]) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')), None,
                    addr(wd['w_hh_t' + sfx]) if w_hh_t else None)
    return _lib.EncoderW(addr(wd['embedding.weight']), lw, addr(wd['encoder2decoder.weight']) if e2d else None,
                         addr(wd['encoder2decoder.bias']) if e2d else None, None, addr(wd['table' + sfx]) if table else None,
                         _lib.SF_ENC_PER_STEP | flags)


def tape_struct(g):
    _lib = _api()[0]
    return _lib.EncoderTape(*(g[k].ptr() if g.get(k) is not None else None for k in ('emb', 'xg', 'gates', 'hs', 'cs')))


def encoder_fwd(wd, H, seq, lens, Lpad, v, flags=0, status=False):
    """sf_encoder_lstm_fwd with SF_ENC_PER_STEP on guarded buffers: (buffers, family kernels, persistent kernels[, status])."""
    _lib, ptr, ws_args, _ = _api()
    B, T = len(lens), max(lens)
    keep = v.gates or not v.table                   # (a backward may follow / the hoisted product needs both)
    g = dict(ctx=Guarded(B, T, H), h=Guarded(B, H), c=Guarded(B, H), hs=Guarded(T + 1, B, H), cs=Guarded(T + 1, B, H),
             gates=Guarded(T, B, 4 * H) if v.gates else None, emb=Guarded(T, B, E) if keep else None,
             xg=Guarded(T, B, 4 * H) if keep else None)
    tp = tape_struct(g)
    w = encoder_w(wd, v.table, flags=flags)
    seq_dev, lens_dev = dev(seq), torch.tensor(lens, dtype=torch.int32, device='cuda')
    rc, fam, pers = profiled(lambda: _lib.lib.sf_encoder_lstm_fwd(
        C.byref(w), B, Lpad, T, E, H, ptr(seq_dev), ptr(lens_dev), g['ctx'].ptr(), g['h'].ptr(), g['c'].ptr(), C.byref(tp),
        drop_arg(v.p), LC.SITE, *ws_args(seq_dev.device)))
    if status:
        return g, fam, pers, rc
    assert rc == 0, rc
    untouched(g, skip=('xg',) if v.table else ())
    if v.table and g['xg'] is not None:
        assert g['xg'].untouched(whole=True), 'with the table nobody writes xg'
    return g, fam, pers


def check_encoder(what, out, w, seq, lens, mask, family, raw_state=False):
    keys = tuple(k for k in LC.ENC_KEYS if out.get(k) is not None)
    for k in keys:
        assert np.isfinite(out[k]).all(), '%s: %s holds non-finite values' % (what, k)
    r64 = LC.encoder_reference(w, seq, lens, mask, torch.float64, raw_state)
    r32 = LC.encoder_reference(w, seq, lens, mask, torch.float32, raw_state)
    LC.compare(what, out, r64, r32, keys, rows=ROWS)
    # exact in every family: the zero initial state, dead rows, ctx = the launch's own h1 times the mirror's mask
    assert not out['hs'][0].any() and not out['cs'][0].any()
    PC.check_state_held(out['hs'], out['cs'], lens)
    T = max(lens)
    want = np.zeros_like(out['ctx'])
    for b, n in enumerate(lens):
        want[b, :n] = out['hs'][1:n + 1, b]
    if mask is not None:
        want = dropped(want, mask)
    assert LC.same_bits(out['ctx'], want), '%s: ctx is not h1 times the mirror\'s mask / +0.0 beyond a length' % what
    assert LC.same_bits(out['c'], out['cs'][T]) and (not raw_state or LC.same_bits(out['h'], out['hs'][T]))
    if family == 'lattice':                         # step 0 stands on the lattice
        m32 = {k: v.astype(F32) for k, v in r32.items()}
        assert LC.same_bits(out['cs'][1], m32['cs'][1]), '%s: c1 of step 0 differs from the exact model' % what
        assert LC.same_bits(out['hs'][1], m32['hs'][1], m32['cs'][1] == 0), '%s: h1 of step 0 differs where it is exact' % what
        if out.get('gates') is not None:
            assert LC.same_bits(out['gates'][0], m32['gates'][0]), '%s: gates of step 0 differ from the exact model' % what


def buffers_np(g):
    return {k: (b.np() if b is not None else None) for k, b in g.items()}


@pytest.mark.parametrize('family', ['lattice', 'plain', 'peaky'])
@pytest.mark.parametrize('case', LC.ENCODER, ids=lambda c: 'H%d-B%d' % c)
def test_encoder_forward_per_step(case, family):
    """sf_encoder_lstm_fwd with SF_ENC_PER_STEP: the step without an input segment, its input half a table row looked up
    through xg_index (Lpad > T) or a row of the hoisted product."""
    H, B = case
    w, wd = encoder_device(H, family)
    kernel = LC.step_kernel(B, H)
    for T in LC.ENC_TS:
        seq, lens = PC.encoder_tokens(B, T, T + 3, vocab=V)
        for v in LC.ENC_VARIANTS:
            what = '%s H%d B%d T%d %s %s p%.1f%s' % (kernel, H, B, T, family, 'table' if v.table else 'hoisted', v.p,
                                                      '' if v.gates else ' nogates')
            g, fam, pers = encoder_fwd(wd, H, seq, lens, T + 3, v)
            assert fam == {kernel: T} and pers == [], (what, fam, pers)
            out = buffers_np(g)
            check_encoder(what, out, w, seq, lens, LC.ctx_mask(v.p, B, T, H), family)
            g2, _, _ = encoder_fwd(wd, H, seq, lens, T + 3, v)
            same_twice(out, buffers_np(g2), LC.ENC_KEYS)


def test_encoder_forward_per_step_raw_state():
    """SF_ENC_RAW_STATE: decoder_init is the raw h_T and ctx is written without dropout, whatever `drop` holds."""
    _lib = _api()[0]
    (H, B), T = LC.ENC_RAW_STATE
    w, wd = encoder_device(H, 'plain')
    seq, lens = PC.encoder_tokens(B, T, T + 3, vocab=V)
    g, fam, pers = encoder_fwd(wd, H, seq, lens, T + 3, LC.EncVariant(True, 0.5, True), flags=_lib.SF_ENC_RAW_STATE)
    assert fam == {LC.step_kernel(B, H): T} and pers == []
    check_encoder('%s H%d B%d T%d raw state' % (LC.step_kernel(B, H), H, B, T), buffers_np(g), w, seq, lens, None, 'plain',
                  raw_state=True)


def test_encoder_per_step_refuses_more_than_64_chunks():
    """H = 1040 is 65 chunks of 16: no per-step kernel covers it (include/sf_hip.h, SF_ENC_PER_STEP).  The entry returns
    SF_ERR_UNSUPPORTED; it has embedded the tokens and filled the zero initial state by then, and written nothing else."""
    H, B, T = LC.ENC_REFUSED_H, 17, 2
    w, wd = encoder_device(H, 'plain')
    seq, lens = PC.encoder_tokens(B, T, T + 3, vocab=V)
    for v in (LC.EncVariant(True, 0.0, True),):
        g, fam, pers, rc = encoder_fwd(wd, H, seq, lens, T + 3, v, status=True)
        assert rc == LC.SF_ERR_UNSUPPORTED and fam == {} and pers == [], (rc, fam, pers)
        for k in ('ctx', 'h', 'c', 'gates', 'xg'):
            assert g[k].untouched(whole=True), k
        for k in ('hs', 'cs'):
            assert not g[k].t[0].any() and bool(torch.isnan(g[k].full[B * H:]).all()), k
    for B in (1, 16, 17, 33):
        assert LC.step_kernel(B, H) == LC.UNSUPPORTED


# ------------------------------------------------------------------------- the speaker decoder's lookup step
@pytest.mark.parametrize('case', LC.SPEAKER, ids=lambda c: 'H%d-B%d' % c)
def test_speaker_decoder_lookup_step(case):
    """sf_speaker_decoder_fwd with xw_table: xg_index = prev_word, xg_index_ld 0; the dropped copy lands in
    cat2[:, H:].  Compared: h1, c1, gates and that copy.  At H = 1024 the step runs (the branch admits H <= 1024) and the
    entry then returns SF_ERR_UNSUPPORTED from its text attention, which covers H <= 512: pinned as found."""
    _lib, ptr, ws_args, _ = _api()
    H, B = case
    Tp, vocab, step_id = LC.SPK_TP, LC.SPK_VOCAB, 3
    kernel = LC.step_kernel(B, H)
    rng = np.random.default_rng([H, B, 83])
    r = lambda *s: dev((rng.standard_normal(s) * H ** -0.5).astype(F32))                # noqa: E731
    rest = dict(w_in=r(H, H), w_out=r(H, 2 * H), w_dec=r(vocab, H), b_dec=r(vocab), ctx=r(B, Tp, H))
    no_mask = torch.zeros(B, Tp, dtype=torch.uint8, device='cuda')
    for family, run in families(H, None):
        d = cell_inputs(family, run, B, H, None, vocab)
        wd = cell_device(dict(d, w_ih=np.zeros((4 * H, 4), F32)))
        table, tok = dev(d['table']), dev(d['tok'])
        h0, c0 = dev(LC.padded(d['h0'], 0)), dev(LC.padded(d['c0'], 0))
        r64, r32 = LC.cell_reference(d, torch.float64), LC.cell_reference(d, torch.float32)
        w = _lib.SpkDecoderW(None, lstm_w(wd), _lib.SoftdotW(addr(rest['w_in']), addr(rest['w_out']), None, None),
                             addr(rest['w_dec']), addr(rest['b_dec']), addr(table), 0, None)
        first = None
        for p in (0.0, 0.5):
            what = '%s lookup H%d B%d %s%d p%.1f' % (kernel, H, B, family, run, p)
            g = dict(gates=Guarded(B, 4 * H), c1=Guarded(B, H), h1=Guarded(B, H), cat2=Guarded(B, 2 * H), t_text=Guarded(B, H),
                     alpha=Guarded(B, Tp), h_tilde=Guarded(B, H), logit=Guarded(B, PC.ldv(vocab)))
            tp = _lib.SpkDecoderTape(None, *(g[k].ptr() for k in ('gates', 'c1', 'h1', 'cat2', 't_text', 'alpha', 'h_tilde',
                                                                  'logit')))
            rc, fam, _ = profiled(lambda: _lib.lib.sf_speaker_decoder_fwd(
                C.byref(w), B, 4, H, Tp, vocab, ptr(tok), ptr(h0), ptr(c0), ptr(rest['ctx']),
                ptr(no_mask), None, C.byref(tp), drop_arg(p), step_id, *ws_args(tok.device)))
            assert fam == {kernel: 1}, (what, fam)
            # (the step comes first; the text attention behind it covers H <= 512 and refuses the rest of the entry above)
            assert rc == (0 if H <= LC.SPK_TEXT_MAX_H else LC.SF_ERR_UNSUPPORTED), (what, rc)
            untouched(g)
            out = {k: g[k].np() for k in ('gates', 'c1', 'h1', 'cat2')}
            mask = orng.dropout_mask(LC.DROP_SEED, 2 * step_id + 1, LC.DROP_ROW0 + np.arange(B), H, p)
            assert LC.same_bits(out['cat2'][:, H:], dropped(out['h1'], mask)), '%s: the dropped copy is not h1 times the mask' % what
            if first is None:
                check_cell(what, out, d, family, r64, r32)
                first = out
            else:
                same_twice(out, first, ('gates', 'c1', 'h1'))


# --------------------------------------------------------------------------- the encoder backward, per step
LSTM_GRADS = ('lstm.weight_ih_l0', 'lstm.weight_hh_l0', 'lstm.bias_ih_l0', 'lstm.bias_hh_l0')


def encoder_bwd(wd, H, lens, tapes, dctx, d_init, d_ct, p, w_hh_t, grads, flags=0):
    """sf_encoder_lstm_bwd with SF_ENC_PER_STEP on the tapes `tapes` (device buffers emb, gates, hs, cs and decoder_init
    'h'): (dgates [T, B, 4H], weight gradients or None, family kernels, persistent kernels)."""
    _lib, ptr, ws_args, _ = _api()
    B, T = len(lens), max(lens)
    dg = Guarded(T, B, 4 * H)
    tp = tape_struct(dict(tapes, xg=dg))
    w = encoder_w(wd, True, w_hh_t, flags)
    gw = None
    gs = None
    if grads:
        gw = {k: torch.zeros_like(wd[k]) for k in LSTM_GRADS + ('encoder2decoder.weight', 'encoder2decoder.bias')}
        gs = _lib.EncoderG(_lib.LstmW(*(addr(gw[k]) for k in LSTM_GRADS), None, None), addr(gw['encoder2decoder.weight']),
                           addr(gw['encoder2decoder.bias']), None, None, 0, -1)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device='cuda')
    _, fam, pers = profiled(lambda: _lib.call(
        'sf_encoder_lstm_bwd', C.byref(w), C.byref(gs) if grads else None, B, T, E, H, ptr(lens_dev), tapes['h'].ptr(),
        ptr(dctx), ptr(d_init), ptr(d_ct), C.byref(tp), drop_arg(p), LC.SITE, *ws_args(lens_dev.device)))
    assert dg.untouched(), 'guard rows of dgates were written'
    return dg.np(), gw, fam, pers


def filled(a):
    g = Guarded(*a.shape)
    g.t.copy_(dev(a))
    return g


def check_encoder_backward(case, family):
    H, B, w_hh_t = case
    kernel = LC.bwd_step_kernel(H, w_hh_t)
    w, wd = encoder_device(H, family)
    rng = np.random.default_rng([H, B, 89])
    for T in LC.BWD_TS:
        seq, lens = PC.encoder_tokens(B, T, T + 3, vocab=V)
        for p in (0.0, 0.5):
            mask = LC.ctx_mask(p, B, T, H)
            # exact: hand-made tapes, d_init NULL, no weight gradients
            tp = LC.exact_backward(B, T, H, lens, seed=T)
            tapes = dict(gates=filled(tp['gates']), cs=filled(tp['cs']), hs=filled(np.zeros((T + 1, B, H), F32)),
                         h=filled(np.zeros((B, H), F32)), emb=None)
            xwd = dict(wd)
            xwd['lstm.weight_hh_l0'] = dev(tp['w_hh'])
            xwd['w_hh_t'] = xwd['lstm.weight_hh_l0'].t().contiguous()
            got, _, fam, pers = encoder_bwd(xwd, H, lens, tapes, dev(tp['dctx']), None, dev(tp['d_ct']), p, w_hh_t, False)
            assert fam == {kernel: T} and pers == [], (fam, pers)
            assert LC.same_bits(got, LC.backward_np(tp, mask, F32)), '%s H%d B%d T%d p%.1f: dgates differ from the exact model' % (
                kernel, H, B, T, p)
            # dense: the tapes of the per-step forward, against float64 autograd
            what = '%s H%d B%d T%d %s p%.1f' % (kernel, H, B, T, family, p)
            g, _, _ = encoder_fwd(wd, H, seq, lens, T + 3, LC.EncVariant(True, p, True))
            up = [rng.standard_normal(s).astype(F32) for s in ((B, T, H), (B, H), (B, H))]
            args = (wd, H, lens, g, dev(up[0]), dev(up[1]), dev(up[2]), p, w_hh_t, True)
            got, gw, fam, pers = encoder_bwd(*args)
            assert fam == {kernel: T} and pers == [], (what, fam, pers)
            assert np.isfinite(got).all()
            g64, dg64 = reference_grads(w, seq, lens, mask, up, torch.float64, False)
            g32, dg32 = reference_grads(w, seq, lens, mask, up, torch.float32, False)
            LC.compare(what, dict(dgates_f=got), dg64, dg32, ('dgates_f',), rows=ROWS)
            for b, n in enumerate(lens):
                assert not got[n:, b].any(), 'dgates of row %d are not zero behind its length' % b
            names = LSTM_GRADS + ('encoder2decoder.weight', 'encoder2decoder.bias')
            GC.compare_grads(gw, {k: g64[k] for k in names}, g32, what=what,
                             blocks={LSTM_GRADS[0]: GC.lstm_blocks(4 * H, cols=E), LSTM_GRADS[1]: GC.lstm_blocks(4 * H, cols=H),
                                     LSTM_GRADS[2]: GC.lstm_blocks(4 * H), LSTM_GRADS[3]: GC.lstm_blocks(4 * H)})
            again, _, _, _ = encoder_bwd(*args)
            assert np.array_equal(LC.bits(got), LC.bits(again)), 'the same backward twice differs'


@pytest.mark.parametrize('family', ['plain', 'peaky'])
@pytest.mark.parametrize('case', LC.BWD_FUSED_CASES, ids=lambda c: 'H%d-B%d' % c[:2])
def test_encoder_backward_fused_step(case, family):
    """sf_encoder_lstm_bwd with SF_ENC_PER_STEP and W_hh^T: lstm_bwd_step_fused_kernel<8> up to H = 256, <16> above; T = 1
    has no dgates_next at all; dctx is random beyond the lengths, where it must reach nothing."""
    check_encoder_backward(case, family)


@pytest.mark.parametrize('family', ['plain', 'peaky'])
@pytest.mark.parametrize('case', LC.BWD_TWO_LAUNCH, ids=lambda c: 'H%d-B%d%s' % (c.H, c.B, '' if c.w_hh_t else '-no_w_hh_t'))
def test_encoder_backward_two_launches(case, family):
    """H > 512 or no W_hh^T: lstm_pw_bwd_kernel (its pass-through written in place over dh1), then dh += dgates W_hh."""
    check_encoder_backward(case, family)


# ----------------------------------------------------------------------------- bidirectional, per step
@pytest.mark.parametrize('case', LC.BIDIR, ids=lambda c: 'H%d-B%d-T%d' % c)
def test_bidirectional_encoder_per_step(case):
    """sf_encoder_bilstm_fwd / _bwd with SF_ENC_PER_STEP at 256 units per direction: the one live user of
    lstm_bwd_step_fused_kernel<8>."""
    _lib, ptr, ws_args, _ = _api()
    H, B, T = case
    w, wd = encoder_device(H, 'plain', True)
    seq, lens = PC.encoder_tokens(B, T, T + 2, vocab=V)
    seq_dev, lens_dev = dev(seq), torch.tensor(lens, dtype=torch.int32, device='cuda')
    p = 0.5
    mask = LC.ctx_mask(p, B, T, 2 * H)
    tapes = [dict(emb=Guarded(T, B, E), xg=Guarded(T, B, 4 * H), gates=Guarded(T, B, 4 * H), hs=Guarded(T + 1, B, H),
                  cs=Guarded(T + 1, B, H)) for _ in range(2)]
    g = dict(ctx=Guarded(B, T, 2 * H), h=Guarded(B, 2 * H), c=Guarded(B, 2 * H))
    ws = [encoder_w(wd, sfx=s, e2d=False) for s in ('', '_reverse')]
    tps = [tape_struct(t) for t in tapes]
    path = C.c_int32(-1)
    _, fam, pers = profiled(lambda: _lib.call(
        'sf_encoder_bilstm_fwd', C.byref(ws[0]), C.byref(ws[1]), addr(wd['encoder2decoder.weight']),
        addr(wd['encoder2decoder.bias']), None, B, T + 2, T, E, H, ptr(seq_dev), ptr(lens_dev), g['ctx'].ptr(), g['h'].ptr(),
        g['c'].ptr(), C.byref(tps[0]), C.byref(tps[1]), drop_arg(p), LC.SITE, C.byref(path), *ws_args(seq_dev.device)))
    kernel = LC.step_kernel(B, H)
    assert fam == {kernel: 2 * T} and pers == [] and path.value == 0, (fam, pers, path.value)
    untouched(g)
    for t in tapes:
        untouched(t, skip=('xg',))
        assert t['xg'].untouched(whole=True)
    what = '%s bidir H%d B%d T%d' % (kernel, H, B, T)
    n = lambda t: t.detach().double().numpy()              # noqa: E731
    models = [PC.encoder_model(w, seq, lens, mask, dt) for dt in (torch.float64, torch.float32)]
    refs = [dict(ctx=n(m['ctx']), h=n(m['decoder_init']), c=n(m['c_t']), **{'%s_%s' % (k, d): n(m[d][k]) for d in 'fr'
                                                                            for k in ('gates', 'hs', 'cs')}) for m in models]
    out = dict(ctx=g['ctx'].np(), h=g['h'].np(), c=g['c'].np(), **{'%s_%s' % (k, d): tapes[i][k].np() for i, d in enumerate('fr')
                                                                    for k in ('gates', 'hs', 'cs')})
    LC.compare(what, out, refs[0], refs[1], tuple(sorted(out)), rows=ROWS)
    PC.check_ctx_beyond_lengths(out['ctx'], lens)
    for d in 'fr':
        PC.check_state_held(out['hs_' + d], out['cs_' + d], lens)
    # backward
    rng = np.random.default_rng([H, B, T, 97])
    up = [rng.standard_normal(s).astype(F32) for s in ((B, T, 2 * H), (B, 2 * H), (B, 2 * H))]
    names = LSTM_GRADS + tuple(k + '_reverse' for k in LSTM_GRADS) + ('encoder2decoder.weight', 'encoder2decoder.bias')
    gw = {k: torch.zeros_like(wd[k]) for k in names}
    gs = [_lib.EncoderG(_lib.LstmW(*(addr(gw[k + s]) for k in LSTM_GRADS), None, None), None, None, None, None, 0, -1)
          for s in ('', '_reverse')]
    ups = [dev(a) for a in up]
    _, fam, pers = profiled(lambda: _lib.call(
        'sf_encoder_bilstm_bwd', C.byref(ws[0]), C.byref(ws[1]), addr(wd['encoder2decoder.weight']), None, C.byref(gs[0]),
        C.byref(gs[1]), addr(gw['encoder2decoder.weight']), addr(gw['encoder2decoder.bias']), B, T, E, H, ptr(lens_dev),
        g['h'].ptr(), ptr(ups[0]), ptr(ups[1]), ptr(ups[2]), C.byref(tps[0]), C.byref(tps[1]), drop_arg(p), LC.SITE,
        C.byref(path), *ws_args(seq_dev.device)))
    bk = LC.bwd_step_kernel(H)
    assert bk == LC.BWD_FUSED % 8 and fam == {bk: 2 * T} and pers == [] and path.value == 0, (fam, pers, path.value)
    for t in tapes:
        untouched(t)
    got = {'dgates_f': tapes[0]['xg'].np(), 'dgates_r': tapes[1]['xg'].np()}
    g64, dg64 = reference_grads(w, seq, lens, mask, up, torch.float64, True)
    g32, dg32 = reference_grads(w, seq, lens, mask, up, torch.float32, True)
    what = '%s bidir H%d B%d T%d' % (bk, H, B, T)
    LC.compare(what, got, dg64, dg32, ('dgates_f', 'dgates_r'), rows=ROWS)
    for v in got.values():
        for b, nb in enumerate(lens):
            assert not v[nb:, b].any(), 'dgates of row %d are not zero behind its length' % b
    GC.compare_grads(gw, {k: g64[k] for k in names}, g32, what=what)
