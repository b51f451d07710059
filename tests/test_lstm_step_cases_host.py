"""Host checks of tests/lstm_step_cases.py (no GPU): the mirror of the two launchers' dispatch reproduces its boundaries
and the tables stand on both sides of each; the exact family is what it claims (float32 and float64 evaluations agree bit
for bit wherever the GPU test asserts bits, every operand column is weighed in some run, the libm facts hold for numpy
float32); and the comparators refuse what a subtly wrong kernel would hand back."""
import numpy as np
import pytest
import torch

from tests import lstm_step_cases as LC
from tests import persist_cases as PC


# ------------------------------------------------------------------------------------------- dispatch
def test_the_mirror_reproduces_the_boundaries():
    assert LC.chunks(256, 256) == 32 and LC.chunks(256, 260) == 33 and LC.chunks(256, 768) == 64
    assert [LC.chunks(h) for h in (16, 512, 528, 1024, 1040)] == [1, 32, 33, 64, 65]
    # total 32 | 33 and 64 | 65, on both sides of B 16 | 17
    assert LC.step_kernel(16, 512) == 'lstm_step_fused_kernel<8>' and LC.step_kernel(16, 528) == 'lstm_step_fused_kernel<16>'
    assert LC.step_kernel(17, 512) == 'lstm_step_wide_kernel<2>' and LC.step_kernel(17, 528) == 'lstm_step_wide_kernel<4>'
    assert LC.step_kernel(16, 1024) == 'lstm_step_fused_kernel<16>' and LC.step_kernel(33, 1024) == 'lstm_step_wide_kernel<4>'
    for B in (1, 16, 17, 33, 129):
        assert LC.step_kernel(B, 1040) == LC.UNSUPPORTED
        assert LC.step_kernel(B, 256, 768) != LC.UNSUPPORTED and LC.step_kernel(B, 256, 784) == LC.UNSUPPORTED
    assert LC.step_kernel(16, 256, 256) == 'lstm_step_fused_kernel<8>' and LC.step_kernel(16, 256, 260) == 'lstm_step_fused_kernel<16>'
    assert LC.step_kernel(17, 256, 256) == 'lstm_step_wide_kernel<2>' and LC.step_kernel(17, 256, 260) == 'lstm_step_wide_kernel<4>'
    assert LC.step_kernel(32, 16, 48) == LC.step_kernel(33, 16, 48) == 'lstm_step_wide_kernel<2>'
    assert LC.step_kernel(4, 24) == LC.UNSUPPORTED and LC.step_kernel(4, 16, 6) == LC.UNSUPPORTED
    assert LC.step_kernel(4, 16, 8, ldx=10) == LC.UNSUPPORTED
    # the cell: I + H <= 1024 takes the fused step
    assert LC.cell_kernel(17, 768, 256) == 'lstm_step_wide_kernel<4>' and LC.cell_kernel(17, 772, 256) == LC.PW_FWD_PREFIX
    assert LC.cell_kernel(100, 4352, 512) == LC.PW_FWD_PREFIX
    # the backward step
    assert [LC.bwd_step_kernel(h) for h in (16, 256, 272, 512, 528)] == [
        'lstm_bwd_step_fused_kernel<8>', 'lstm_bwd_step_fused_kernel<8>', 'lstm_bwd_step_fused_kernel<16>',
        'lstm_bwd_step_fused_kernel<16>', 'lstm_pw_bwd_kernel']
    assert LC.bwd_step_kernel(512, w_hh_t=False) == 'lstm_pw_bwd_kernel'


def test_the_tables_name_every_kernel_and_stand_on_both_sides_of_every_edge():
    want = {'lstm_step_fused_kernel<8>', 'lstm_step_fused_kernel<16>', 'lstm_step_wide_kernel<2>', 'lstm_step_wide_kernel<4>',
            'lstm_bwd_step_fused_kernel<8>', 'lstm_bwd_step_fused_kernel<16>', 'lstm_pw_bwd_kernel'}
    got = LC.all_kernels()
    assert want <= got and LC.UNSUPPORTED not in got
    ks = sorted(c.KS for c in LC.POINTWISE)
    assert 1 in ks and 8 in ks and len({k for k in ks if 1 < k != 8}) >= 2
    assert LC.Pw(100, 4352, 512, 8) in LC.POINTWISE
    assert got - want == {LC.PW_FWD % k for k in ks}
    for name, lo, hi, values in LC.boundaries():
        assert lo in values and hi in values, name
    for c in LC.CELL:
        assert c.I + c.H <= LC.CELL_FUSED_MAX and c.H in LC.HS and c.B <= 33
    for c in LC.POINTWISE:
        assert c.I + c.H > LC.CELL_FUSED_MAX and c.H in LC.HS
    assert LC.step_kernel(17, LC.ENC_REFUSED_H) == LC.UNSUPPORTED
    assert {LC.step_kernel(c.B, c.H) for c in LC.BIDIR} == {'lstm_step_fused_kernel<8>', 'lstm_step_wide_kernel<2>'}
    assert {LC.bwd_step_kernel(c.H) for c in LC.BIDIR} == {'lstm_bwd_step_fused_kernel<8>'}


# --------------------------------------------------------------------------------------- exact family
def test_the_libm_facts_hold_for_numpy_float32():
    assert LC.libm_facts(np.exp, np.tanh) == []
    f = np.float32
    assert f(1) / (f(1) + np.exp(f(-40))) == f(1) and f(1) / (f(1) + np.exp(f(0))) == f(0.5)


EXACT_SHAPES = sorted({(c.H, c.I) for c in LC.CELL} | {(c.H, None) for c in LC.SPEAKER} | {(c.H, c.I) for c in LC.POINTWISE
                                                                                          if c.B <= 33},
                      key=lambda s: (s[0], s[1] or 0))


@pytest.mark.parametrize('H,I', EXACT_SHAPES, ids=lambda v: str(v))
def test_exact_family_forward(H, I):
    """Pre-activations are single terms on {0, +-40} (minus on gate g only); float32 and float64 agree bit for bit on
    the gates, c1 and the exact part of h1; every operand column is weighed in a run in which it carries data."""
    vocab = None if I else LC.SPK_VOCAB
    assert LC.exact_columns_covered(H, I, vocab)
    frac = []
    for run in range(LC.exact_runs(H, I)):
        d = LC.exact_cell(5, H, I, run, vocab)
        for k in ('w_hh', 'w_ih'):
            if d[k] is not None:
                assert set(np.unique(d[k])) <= {-1.0, 0.0, 1.0}
        w = np.concatenate([d[k] for k in ('w_ih', 'w_hh') if d[k] is not None], 1)
        assert ((w != 0).sum(1) == 1).all()
        pre = d['b_ih'] + d['b_hh'] + (d['table'][d['tok']] if vocab else 0)
        for a, wk in ((d['x'], d['w_ih']), (d['h0'], d['w_hh'])):
            if a is not None:
                pre = pre + a.astype(np.float64) @ wk.astype(np.float64).T
        assert set(np.unique(pre)) <= {-40.0, 0.0, 40.0}
        assert (pre[:, :2 * H] >= 0).all() and (pre[:, 3 * H:] >= 0).all() and (pre[:, 2 * H:3 * H] < 0).any()
        r32, r64 = LC.cell_np(d, np.float32), LC.cell_np(d, np.float64)
        assert r32['gates'].dtype == np.float32
        for k in ('gates', 'c1'):
            assert LC.same_bits(r32[k], r64[k]), k
        assert np.array_equal(r32['exact'], r64['exact']) and LC.same_bits(r32['h1'], r64['h1'], r64['exact'])
        assert set(np.unique(r64['gates'][:, :2 * H])) <= {0.5, 1.0} and set(np.unique(r64['gates'][:, 2 * H:3 * H])) <= {-1.0, 0.0, 1.0}
        frac.append(r64['exact'].mean())
        if vocab:
            assert len(np.unique(d['table'], axis=0)) > 1 and (d['b_ih'] != 0).any() and (d['b_hh'] != 0).any()
    assert min(frac) > 0.5


@pytest.mark.parametrize('H', sorted({c.H for c in LC.ENCODER}))
def test_lattice_encoder_step_0_is_exact(H):
    w = LC.encoder_weights(H, 'lattice')
    seq, lens = PC.encoder_tokens(5, 2, 4, vocab=LC.ENC_VOCAB)
    r32 = LC.encoder_reference(w, seq, lens, None, torch.float32)
    r64 = LC.encoder_reference(w, seq, lens, None, torch.float64)
    assert LC.same_bits(r32['gates'][0], r64['gates'][0]) and LC.same_bits(r32['cs'][1], r64['cs'][1])
    table = LC.xw_table(w)
    assert set(np.unique(table)) <= {-40.0, 0.0, 40.0} and len(np.unique(table[4:], axis=0)) > 1
    nz = (table != 0).any(0).astype(int) + (w['lstm.bias_ih_l0'] != 0) + (w['lstm.bias_hh_l0'] != 0)
    assert nz.max() == 1
    zero = r64['cs'][1] == 0
    assert LC.same_bits(r32['hs'][1], r64['hs'][1], zero) and 0.2 < zero.mean() < 0.9


@pytest.mark.parametrize('H,B,T', [(16, 17, 4), (256, 16, 4), (272, 17, 4), (512, 17, 4), (528, 17, 4), (512, 1, 1)])
def test_exact_family_backward(H, B, T):
    """float32 and float64 evaluations of the hand-made tapes agree on every bit of dgates, with and without the scale-2
    dropout mask: every intermediate fits float32, so no summation order or fused multiply-add can change a bit."""
    _, lens = PC.encoder_tokens(B, T, T, vocab=LC.ENC_VOCAB)
    tp = LC.exact_backward(B, T, H, lens)
    assert ((tp['w_hh'] != 0).sum(0) == 1).all() and set(np.unique(tp['w_hh'])) == {0.0, 1.0}
    for p in (0.0, 0.5):
        mask = LC.ctx_mask(p, B, T, H)
        r32, r64 = LC.backward_np(tp, mask, np.float32), LC.backward_np(tp, mask, np.float64)
        assert r32.dtype == np.float32 and LC.same_bits(r32, r64)
        for b, n in enumerate(lens):
            assert not r64[n:, b].any()
        assert (r64[0] != 0).mean() > 0.1
        assert not LC.same_bits(LC.backward_np(tp, mask, np.float32, leak_dctx=True), r64) or min(lens) == T


def test_exact_cell_backward():
    for B, H, I in ((3, 16, 48), (17, 512, 4352)):
        d, r32, r64 = LC.exact_cell_backward(B, H, I)
        for k in ('dx', 'dh0', 'dc0'):
            assert LC.same_bits(r32[k], r64[k]) and r64[k].any(), k
        assert ((d['w_ih'] != 0).sum(0) == 1).all() and ((d['w_hh'] != 0).sum(0) == 1).all()


# ------------------------------------------------------------------- the comparators refuse planted errors
def _refused(got, r64, r32, keys):
    with pytest.raises(AssertionError):
        LC.compare('planted', got, r64, r32, keys)
    return True


CELL_KEYS = ('gates', 'c1', 'h1')


@pytest.mark.parametrize('family', ['exact', 'plain', 'peaky'])
def test_planted_errors_in_the_forward_step_are_refused(family):
    B, H, I = 33, 256, 260
    d = LC.exact_cell(B, H, I, 1) if family == 'exact' else LC.dense_cell(B, H, I, family == 'peaky')
    r64 = {k: np.asarray(v, np.float64) for k, v in LC.cell_np(d).items()}
    r32 = {k: np.asarray(v, np.float64) for k, v in LC.cell_np(d, np.float32).items()}
    LC.compare('clean', r32, r64, r32, CELL_KEYS)
    planted = {'two gates swapped in one tile': LC.cell_np(d, np.float32, swap_gates=(0, 1)),
               'gates g and o swapped in one tile': LC.cell_np(d, np.float32, swap_gates=(2, 3))}
    for c in range(LC.chunks(H, I)):
        planted['chunk %d dropped' % c] = LC.cell_np(d, np.float32, drop_chunk=c)
    shifted = {k: v.copy() for k, v in LC.cell_np(d, np.float32).items()}
    for k in CELL_KEYS:
        shifted[k][16:32] = shifted[k][17:33]
    planted['rows 16.. of a 32-row tile shifted by one'] = shifted
    for name, got in planted.items():
        if family == 'exact':
            # (a chunk whose columns are all held at zero in this run shows in the run that holds the other half)
            other = LC.exact_cell(B, H, I, 0)
            hit = not all(LC.same_bits(got[k], r64[k]) for k in CELL_KEYS)
            if not hit and name.startswith('chunk'):
                c = int(name.split()[1])
                hit = not LC.same_bits(LC.cell_np(other, np.float32, drop_chunk=c)['gates'], LC.cell_np(other)['gates'])
            assert hit, name
        else:
            assert _refused(got, r64, r32, CELL_KEYS), name


@pytest.mark.parametrize('family', ['lattice', 'plain'])
def test_a_dead_row_advanced_is_refused(family):
    B, T, H = 5, 4, 16
    w = LC.encoder_weights(H, family)
    seq, lens = PC.encoder_tokens(B, T, T + 1, vocab=LC.ENC_VOCAB)
    seq[:, :T] = np.where(seq[:, :T] == 0, 5, seq[:, :T])            # (a token behind each length for the planted step)
    row = next(b for b, n in enumerate(lens) if n < T)
    r64 = LC.encoder_reference(w, seq, lens, None, torch.float64)
    r32 = LC.encoder_reference(w, seq, lens, None, torch.float32)
    LC.compare('clean', r32, r64, r32, LC.ENC_KEYS)
    PC.check_state_held(r32['hs'], r32['cs'], lens)
    got = LC.encoder_reference(w, seq, lens, None, torch.float32, advance_row=row)
    assert _refused(got, r64, r32, LC.ENC_KEYS)
    with pytest.raises(AssertionError):
        PC.check_state_held(got['hs'], got['cs'], lens)
    with pytest.raises(AssertionError):
        PC.check_ctx_beyond_lengths(got['ctx'], lens)


def test_dctx_beyond_a_length_added_is_refused():
    B, T, H = 17, 4, 16
    _, lens = PC.encoder_tokens(B, T, T, vocab=LC.ENC_VOCAB)
    tp = LC.exact_backward(B, T, H, lens)
    r64, r32 = LC.backward_np(tp), LC.backward_np(tp, dtype=np.float32)
    got = LC.backward_np(tp, dtype=np.float32, leak_dctx=True)
    assert LC.same_bits(r32, r64) and not LC.same_bits(got, r64)
    assert _refused(dict(dgates=got), dict(dgates=r64), dict(dgates=r32.astype(np.float64)), ('dgates',))
    rng = np.random.default_rng(3)
    sig = lambda n: 1 / (1 + np.exp(-rng.standard_normal((T, B, n * H))))      # noqa: E731
    dense = dict(tp, gates=np.concatenate([sig(2), np.tanh(rng.standard_normal((T, B, H))), sig(1)], 2).astype(np.float32),
                 cs=rng.standard_normal((T + 1, B, H)).astype(np.float32), dctx=rng.standard_normal((B, T, H)).astype(np.float32),
                 w_hh=(rng.standard_normal((4 * H, H)) / 4).astype(np.float32))
    r64, r32 = LC.backward_np(dense), LC.backward_np(dense, dtype=np.float32).astype(np.float64)
    LC.compare('clean', dict(dgates=r32), dict(dgates=r64), dict(dgates=r32), ('dgates',))
    got = LC.backward_np(dense, dtype=np.float32, leak_dctx=True)
    assert _refused(dict(dgates=got), dict(dgates=r64), dict(dgates=r32), ('dgates',))
