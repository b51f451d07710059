"""GPU: the RECURRENT half of the decoder LSTM's gates as a row (include/sf_hip.h: sf_gate_rows_recurrent_use;
csrc/sf_api_follower.hip: tail_proj, episode_gate_rows) -- launch (2) of step t carries the product blocks of
xg_h = h1 W_hh^T + b_ih + b_hh (csrc/sf_attention.hip: pair_proj_score_hh_kernel) and the cell of step t + 1 is a product
over the location columns alone, K = LOC, that adds three rows (csrc/sf_gemm.hip: lstm_step_rows_kernel).

Checked here, at the full model dimensions with tiny feature tables (NVP = 24, S = 3):
  * the cell alone (sf_lstm_cell_rows3_fwd) against float64 at every row-block edge, and at one small shape;
  * xg_h as the rollout left it in the workspace, and on caller buffers, against float64;
  * the chain with the switch on against off and against the numpy oracle; the kernels each leg launches;
  * capture and replay, a padded sample, and every case that declines."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402
from tests.follower_models import full_size_models                    # noqa: E402
from tests.test_gpu_gate_rows import _edge_batch, _run                # noqa: E402
from tests.test_gpu_gate_rows_attended import NVP, S, _models, _reference   # noqa: E402


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('B,H,IMG,LOC', [(1, 512, 2048, 128), (16, 512, 2048, 128), (17, 512, 2048, 128), (32, 512, 2048, 128),
                                         (33, 512, 2048, 128), (100, 512, 2048, 128), (33, 32, 16, 16)])
def test_cell_on_the_location_columns_with_three_rows_against_float64(B, H, IMG, LOC):
    """sf_lstm_cell_rows3_fwd with x_col0 = F + IMG: gates = xin[:, F+IMG:2F] W_ih[:, F+IMG:2F]^T + xg_h + xg + xg2 (the
    biases and the recurrent product are inside xg_h, an input here), against float64.  The bound is the one
    test_cell_on_the_location_columns_with_both_rows_against_float64 holds its cell to, over the one product this kernel
    forms: pre-activations within 2.5e-7 * sum |a| |b| + 2^-23 * 6 * max |pre|, c1 and h1 within 4 x (that (1 + |c0|) +
    2^-22 (1 + |c0|)), the activated gates (slope <= 1) within 4 x (that + 2^-22).  (H 32, LOC 16: one K chunk, seven of
    the eight waves idle.)  Every buffer has three rows past B: inputs hold 1e4 there, outputs NaN, which must stay."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import ptr, ws_args
    F, N, P = IMG + LOC, 4 * H, 3
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu')
    g.manual_seed(300 + B + H)
    rn = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    x, h0, c0 = rn(B, 2 * F), rn(B, H) * 0.5, rn(B, H)
    w_ih, w_hh, b_ih, b_hh = rn(N, 2 * F) * 0.05, rn(N, H) * 0.05, rn(N) * 0.1, rn(N) * 0.1
    xg, xg2 = rn(B, N) * 0.5, rn(B, N) * 0.5
    xg_h = torch.from_numpy((_f64(h0) @ _f64(w_hh).T + _f64(b_ih) + _f64(b_hh)).astype(np.float32))
    pad = lambda t, v: torch.cat([t, torch.full((P,) + tuple(t.shape[1:]), v)]).to(dev).contiguous()   # noqa: E731
    X, H0, C0, XG, XG2, XGH = (pad(t, 1e4) for t in (x, h0, c0, xg, xg2, xg_h))
    WI, WH, BI, BH = (t.to(dev).contiguous() for t in (w_ih, w_hh, b_ih, b_hh))
    w = _lib.LstmW(WI.data_ptr(), WH.data_ptr(), BI.data_ptr(), BH.data_ptr())
    H1, C1, G = (torch.full((B + P, n), float('nan'), device=dev) for n in (H, H, N))
    _lib.check(_lib.lib.sf_lstm_cell_rows3_fwd(C.byref(w), B, 2 * F, H, ptr(X), 2 * F, F + IMG, ptr(XG), ptr(XG2), ptr(XGH),
                                               ptr(H0), ptr(C0), ptr(H1), ptr(C1), ptr(G), *ws_args(dev)),
               'sf_lstm_cell_rows3_fwd')
    torch.cuda.synchronize()
    a, wl = _f64(x)[:, F + IMG:], _f64(w_ih)[:, F + IMG:]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))                          # noqa: E731
    pre = a @ wl.T + _f64(xg_h) + _f64(xg) + _f64(xg2)
    perr = 2.5e-7 * (np.abs(a) @ np.abs(wl).T) + 2.0 ** -23 * 6 * np.abs(pre).max()
    i, f, gg, o = sig(pre[:, :H]), sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
    c1 = f * _f64(c0) + i * gg
    h1 = o * np.tanh(c1)
    pe = perr.reshape(B, 4, H).max(axis=1)
    bound = 4 * (pe * (1 + np.abs(_f64(c0))) + 2.0 ** -22 * (1 + np.abs(_f64(c0))))
    ec, eh = np.abs(_f64(C1[:B]) - c1), np.abs(_f64(H1[:B]) - h1)
    eg = np.abs(_f64(G[:B]) - np.concatenate([i, f, gg, o], axis=1))
    print('[cell three rows B=%d H=%d] c1 max err %.3e (err / bound %.3f), h1 %.3e (%.3f), gates %.3e (%.3f)'
          % (B, H, ec.max(), float((ec / bound).max()), eh.max(), float((eh / bound).max()), eg.max(),
             float((eg / (4 * (perr + 2.0 ** -22))).max())))
    assert np.all(ec <= bound) and np.all(eh <= bound) and np.all(eg <= 4 * (perr + 2.0 ** -22))
    assert bool(torch.isnan(H1[B:]).all()) and bool(torch.isnan(C1[B:]).all()) and bool(torch.isnan(G[B:]).all())
    # a shape outside the rule is refused before anything is launched: K = LOC + IMG columns left (x_col0 = F)
    if IMG + LOC > 256:
        assert _lib.lib.sf_lstm_cell_rows3_fwd(C.byref(w), B, 2 * F, H, ptr(X), 2 * F, F, ptr(XG), ptr(XG2), ptr(XGH), ptr(H0),
                                               ptr(C0), ptr(H1), ptr(C1), None, *ws_args(dev)) == _lib.SF_ERR_UNSUPPORTED


def _world(B, pad_rows=()):
    from speaker_follower_amd import features, follower
    fb = _edge_batch(B, S)
    for r in pad_rows:
        fb.vp[1:, r] = -1
    table = synth.feature_table(5, NVP)
    store = features.FeatureStore(table)
    return fb, table, store, follower.DeviceFollowerBatch.from_synth(fb)


def _engine(enc, dec, store, rec):
    from speaker_follower_amd import follower
    eng = follower.FollowerEngine(enc, dec, store)
    eng.project, eng.gate_rows_recurrent = True, rec
    return eng


def _pair(enc, dec, store, batch, feedback='argmax', expect=True):
    """The same rollout with the recurrent row off and on (both gate-space rows on in both); the step counter moves by
    S - 1 when on (where `expect`) and stands still when off."""
    from speaker_follower_amd import _lib
    steps = _lib.lib.sf_gate_rows_recurrent_steps
    n0 = steps()
    off = _run(_engine(enc, dec, store, False), batch, S, feedback)
    assert off.gate_rows_attended and not off.gate_rows_recurrent and steps() == n0
    on = _run(_engine(enc, dec, store, True), batch, S, feedback)
    assert on.gate_rows_attended and bool(on.gate_rows_recurrent) == expect and steps() - n0 == (S - 1 if expect else 0)
    return off, on


def _bits(st):
    return st.logits.clone(), st.actions.clone(), st.h.clone(), st.c.clone(), st.tape['alpha_v'].clone()


@pytest.mark.parametrize('B', [1, 17, 100])
def test_row_in_the_workspace_and_on_caller_buffers_against_float64(B):
    """xg_h as launch (2) of steps 0 and 1 left it: episode_gate_rows carves xg_next[0..1], xg_f[0..1], xg_h[0..1] off the
    front of the stream's workspace, each B * 4H floats rounded up to 64, and step t writes buffer t & 1 (nothing writes
    behind the last step).  Against h1[t] W_hh^T + b_ih + b_hh in float64 from the tape's own fp32 h1, every entry within
    2.5e-7 * sum |a| |b| over the 512 product terms: the project's bound for fp32 products (the biases add nothing to
    it).  The same product on caller buffers (sf_debug_recurrent_row) gives the same bits."""
    from speaker_follower_amd import _lib, runtime
    from speaker_follower_amd.runtime import ptr, stream
    enc, dec, _, dec_w = _models()
    _, _, store, batch = _world(B)
    on = _run(_engine(enc, dec, store, True), batch, S)
    assert on.gate_rows_recurrent
    H = dec.hidden_size
    H4 = 4 * H
    row = (B * H4 + 63) // 64 * 64
    dev = torch.device('cuda', torch.cuda.current_device())
    ws = runtime.workspace(dev).view(torch.float32)
    w_hh = np.asarray(dec_w['lstm.weight_hh'], np.float64)
    bias = np.asarray(dec_w['lstm.bias_ih'], np.float64) + np.asarray(dec_w['lstm.bias_hh'], np.float64)
    lw = _lib.LstmW(dec.lstm.weight_ih.data_ptr(), dec.lstm.weight_hh.data_ptr(), dec.lstm.bias_ih.data_ptr(),
                    dec.lstm.bias_hh.data_ptr())
    for k in (0, 1):
        got = ws[(4 + k) * row:(4 + k) * row + B * H4].reshape(B, H4).clone()
        h1 = on.tape['h1'][k]
        a = _f64(h1)
        want, bound = a @ w_hh.T + bias, 2.5e-7 * (np.abs(a) @ np.abs(w_hh).T)
        err = np.abs(_f64(got) - want)
        print('[xg_h B=%d step %d] max err %.3e, max err / bound %.3f, max |entry| %.3f'
              % (B, k, err.max(), float((err / bound).max()), np.abs(want).max()))
        assert np.all(err <= bound)
        alone = torch.full((B, H4), float('nan'), device=dev)
        _lib.check(_lib.lib.sf_debug_recurrent_row(C.byref(lw), B, H, ptr(h1.contiguous()), H, ptr(alone), stream()),
                   'sf_debug_recurrent_row')
        torch.cuda.synchronize()
        assert torch.equal(alone, got)


@pytest.mark.parametrize('feedback', ['argmax', 'sample'])
@pytest.mark.parametrize('B', [1, 17, 100])
def test_chain_on_against_off_and_the_oracle(B, feedback):
    enc, dec, enc_w, dec_w = _models()
    fb, table, store, batch = _world(B)
    off, on = _pair(enc, dec, store, batch, feedback)
    lu, lg = off.logits.cpu().numpy(), on.logits.cpu().numpy()
    fin = np.isfinite(lu)
    assert np.array_equal(fin, np.isfinite(lg))                    # finite logits in the same places
    scale = float(np.abs(lu[fin]).max())
    d = float(np.abs(lg[fin] - lu[fin]).max())
    print('[recurrent row, %s B=%d] max |logit| %.2f, on vs off %.2e (bound %.2e)' % (feedback, B, scale, d, 3e-5 * max(scale, 1.0)))
    assert torch.equal(on.actions, off.actions)
    assert 0 < d <= 3e-5 * max(scale, 1.0)                         # (> 0: the three-row cell ran, in another summation order)
    assert torch.equal(on.logits[0], off.logits[0])                # step 0 keeps its full product
    dl = abs(float(on.loss_buf) - float(off.loss_buf))
    assert dl <= 1e-5 * max(1.0, abs(float(off.loss_buf)))         # (the bound the attended rows' comparison holds the loss to)
    if feedback == 'sample':                                        # (the reference's torch RNG stream cannot be reproduced)
        return
    ref = _reference((B, feedback), fb, table, enc_w, dec_w)
    n = len(ref['logits'])
    for st, l in ((off, lu), (on, lg)):
        assert np.array_equal(st.actions.cpu().numpy()[:n], ref['actions'])
        for t in range(n):
            a = ref['logits'][t].shape[1]
            ok = np.isfinite(ref['logits'][t])
            assert float(np.abs(l[t][:, :a][ok] - ref['logits'][t][ok]).max()) <= 1e-4


def _names(eng, batch):
    from speaker_follower_amd import _lib
    with torch.no_grad():
        eng.rollout(batch, S, 'argmax', train=False)
        torch.cuda.synchronize()
        with _lib.kernel_profile() as prof:
            st = eng.rollout(batch, S, 'argmax', train=False)
            torch.cuda.synchronize()
    return st, {k: v['calls'] for k, v in prof.rows.items()}


def test_kernel_names_of_both_legs():
    """On: behind step 0 every cell is lstm_step_rows_kernel<1> (no lstm_step_wide_kernel<4> over K = 640), launch (2) of
    every step but the last is pair_proj_score_hh_kernel<4> at B = 100, and the last step's is pair_proj_score_kernel<2>: it
    carries no product blocks.  Off: the names the attended rows alone launch, and nothing else."""
    enc, dec, _, _ = _models()
    _, _, store, batch = _world(100)
    st, on = _names(_engine(enc, dec, store, True), batch)
    assert st.gate_rows_recurrent
    assert on.get('lstm_step_rows_kernel<1>') == S - 1 and 'lstm_step_wide_kernel<4>' not in on
    assert on.get('pair_proj_score_hh_kernel<4>') == S - 1 and on.get('pair_proj_score_kernel<2>') == 1
    st, off = _names(_engine(enc, dec, store, False), batch)
    assert not st.gate_rows_recurrent
    assert off.get('lstm_step_wide_kernel<4>') == S - 1 and off.get('pair_proj_score_kernel<2>') == S
    assert not [k for k in off if 'lstm_step_rows_kernel' in k or 'pair_proj_score_hh_kernel' in k]
    same = lambda d: {k: v for k, v in d.items() if 'lstm_step_' not in k and 'pair_proj_score' not in k}   # noqa: E731
    assert same(on) == same(off)                                    # every other launch is the same in both legs


def test_capture_replays_bit_equal_to_the_eager_rollout():
    """Three replays give the same bits, and the bits of an eager rollout: a ping-pong or stale-row mistake would show in
    the second replay, which starts with the rows the first one left."""
    enc, dec, _, _ = _models()
    _, _, store, batch = _world(17)
    replay, gst = _engine(enc, dec, store, True).capture(batch, S, 'argmax')
    assert gst.gate_rows_attended and gst.gate_rows_recurrent
    outs = []
    for _ in range(3):
        replay()
        torch.cuda.synchronize()
        outs.append(_bits(gst))
    assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
    ref = _run(_engine(enc, dec, store, True), batch, S)
    assert ref.gate_rows_recurrent and all(torch.equal(a, b) for a, b in zip(outs[0], _bits(ref)))


def test_padded_sample_leaves_the_live_rows_bits_alone():
    """Rows 1 and 5 padded (vp < 0) from step 1 on: every live row's logits, state and attention weights are, bit for bit,
    those of the batch without padding -- no kernel of the chain mixes rows -- and on against off holds its bound."""
    enc, dec, _, _ = _models()
    B = 17
    live = [b for b in range(B) if b not in (1, 5)]
    _, _, store, batch = _world(B)
    _, _, pstore, pbatch = _world(B, pad_rows=(1, 5))
    plain = _run(_engine(enc, dec, store, True), batch, S)
    off, on = _pair(enc, dec, pstore, pbatch)
    assert plain.gate_rows_recurrent
    for a, b in ((plain.logits, on.logits), (plain.tape['h1'], on.tape['h1']), (plain.tape['c1'], on.tape['c1']),
                 (plain.tape['alpha_v'], on.tape['alpha_v'])):
        assert torch.equal(a[:, live], b[:, live])
    fin = torch.isfinite(off.logits)
    assert torch.equal(fin, torch.isfinite(on.logits)) and torch.equal(on.actions, off.actions)
    assert float((on.logits[fin] - off.logits[fin]).abs().max()) <= 3e-5 * max(1.0, float(off.logits[fin].abs().max()))


@pytest.mark.parametrize('case', ['attended False', 'bf16', 'late partials', 'workspace'])
def test_declining_cases_reproduce_the_switch_off_bits(case):
    """Every case that declines launches what the switch-off leg launches: the same bits, the counter standing still.
    'workspace': at B = 160 the stream's workspace holds the four rows of both halves but not six (episode_gate_rows: the
    capacity rule is six rows within an eighth of what is left), so the attended rows run and the recurrent row does not."""
    from speaker_follower_amd import _lib
    enc, dec, _, _ = _models()
    _, _, store, batch = _world(160 if case == 'workspace' else 17)
    out = {}
    for rec in (True, False):
        eng = _engine(enc, dec, store, rec)
        if case == 'attended False':
            eng.gate_rows_attended = False
        elif case == 'bf16':
            eng.gate_weights = 'bf16'
        n0 = _lib.lib.sf_gate_rows_recurrent_steps()
        if case == 'late partials':
            _lib.lib.sf_debug_projected_partials_late(1)
            try:
                st = _run(eng, batch, S)
            finally:
                _lib.lib.sf_debug_projected_partials_late(0)
        else:
            st = _run(eng, batch, S)
        assert not st.gate_rows_recurrent and _lib.lib.sf_gate_rows_recurrent_steps() == n0
        assert bool(st.gate_rows_attended) == (case == 'workspace')
        out[rec] = _bits(st)
    assert all(torch.equal(a, b) for a, b in zip(out[True], out[False]))


@pytest.mark.parametrize('grad', [True, False])
def test_training_with_dropout_reproduces_the_switch_off_bits(grad):
    """A train-mode rollout (dropout on; with a tape for the backward, or under no_grad) never runs the folded text stage,
    so the projected chain and every row that rides on it decline as they do for the attended row -- with the tables
    registered (an inference rollout has just built and used them), so it is the policy that declines.  The dropout masks
    are a function of the engine's `dropout_seed` and its site numbering: two fresh engines with the same seed draw the
    same masks, so the switch-on leg is held to the switch-off leg bit for bit -- logits, actions, h, c, alpha_v, loss --
    and the counters stand still."""
    from speaker_follower_amd import _lib
    enc, dec, _, _ = full_size_models(83)
    _, _, store, batch = _world(17)
    enc.eval(); dec.eval()
    assert _run(_engine(enc, dec, store, True), batch, S).gate_rows_recurrent
    enc.train(); dec.train()
    out = {}
    try:
        for rec in (True, False):
            eng = _engine(enc, dec, store, rec)
            eng.dropout_seed = 4242
            n0, a0 = _lib.lib.sf_gate_rows_recurrent_steps(), _lib.lib.sf_gate_rows_attended_steps()
            with torch.enable_grad() if grad else torch.no_grad():
                st = eng.rollout(batch, S, 'argmax', train=True)
            torch.cuda.synchronize()
            assert not st.gate_rows_recurrent and not st.gate_rows_attended
            assert _lib.lib.sf_gate_rows_recurrent_steps() == n0 and _lib.lib.sf_gate_rows_attended_steps() == a0
            out[rec] = tuple(t.detach() for t in _bits(st)) + (st.loss.detach().clone(),)
    finally:
        enc.eval(); dec.eval()
    assert all(torch.equal(a, b) for a, b in zip(out[True], out[False]))
    # (the masks are on: another seed gives other bits)
    other = _engine(enc, dec, store, True)
    other.dropout_seed = 4243
    enc.train(); dec.train()
    try:
        with torch.enable_grad() if grad else torch.no_grad():
            st = other.rollout(batch, S, 'argmax', train=True)
        torch.cuda.synchronize()
    finally:
        enc.eval(); dec.eval()
    assert not torch.equal(st.logits.detach(), out[True][0])
