"""GPU: GATE-SPACE ROWS for the attended half of the decoder LSTM's input (include/sf_hip.h: sf_gate_rows_attended_build;
csrc/sf_api_follower.hip: episode_gate_rows, tail_proj) -- launch (1)'s attention partials sum rows of GF = table
W_ih[:, F:F+IMG]^T, launch (2)'s merge leaves the normalised 4H part as a [B, 4H] row, and the next step's gate product runs
over [f_loc | h0], K = LOC + H, its cell adding that row and the action half's.

Checked here, at the full model dimensions with peaky weights and tiny feature tables:
  * GF, every entry, against float64 numpy formed from the same fp32 weights, in one chunk and in several;
  * the cell alone (sf_lstm_cell_rows_fwd) on the location columns [F+IMG, 2F) with both rows against float64;
  * the chain with the attended rows on against off (`gate_rows` on in both) and against the numpy oracle, for argmax,
    teacher and sample feedback at B = 1, 16 and 100, V = 36 and the smallest V the chain takes, a padded sample included,
    (the projected chain itself declines at H = 256, so no chain case with 4H != IMG can be run: the widths are held
    apart on the host, tests/test_gate_rows_attended_host.py);
  * the policy: capture and replay, the in-place refresh of both tables, and every case that declines."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402
from oracle import np_env, np_model                                   # noqa: E402
from tests.follower_models import full_size_models                    # noqa: E402
from tests.test_gpu_gate_rows import _edge_batch, _run                # noqa: E402

NVP = 24
S = 3
_cache = {}


def _models(seed=77):
    if seed not in _cache:
        _cache[seed] = full_size_models(seed)
    return _cache[seed]


def _w_ih64(dec_w):
    return np.asarray(dec_w['lstm.weight_ih'], np.float64)          # [4H, 2F]


@pytest.mark.parametrize('n_vp,chunk', [(1, 0), (3, 0), (15, 0), (30, 512), (5, 64)])
def test_table_matches_float64_numpy(n_vp, chunk):
    """Every entry of GF within 2.5e-7 * sum |a| |b| of the float64 product of the same fp32 weights: the bound
    tests/test_gpu_gate_rows.py holds GU to, at its table sizes (n_vp = 15 is the smallest table on the many-row kernel;
    chunk > 0 builds in several chunks, smaller than the table)."""
    from speaker_follower_amd import _lib, features
    enc, dec, _, dec_w = _models()
    table = synth.feature_table(5, n_vp)
    store = features.FeatureStore(table)
    _lib.lib.sf_debug_projected_chunk_rows(chunk)
    try:
        hit = store.gate_rows(dec)
        torch.cuda.synchronize()
    finally:
        _lib.lib.sf_debug_projected_chunk_rows(0)
    H, IMG, LOC = synth.FULL.hidden, synth.FULL.img, 128
    F = IMG + LOC
    assert hit['builds'] == 1 and len(hit['bufs']) == 2 and hit['attended'] is not None
    gf = hit['attended']['buf'].cpu().numpy().astype(np.float64)
    assert gf.shape == (n_vp * 36, 4 * H)
    x = table.reshape(-1, IMG).astype(np.float64)
    wt = _w_ih64(dec_w)[:, F:F + IMG]
    want, bound = x @ wt.T, 2.5e-7 * (np.abs(x) @ np.abs(wt).T)
    err = np.abs(gf - want)
    print('[GF n_vp=%d] max err %.3e, max err / bound %.3f, max |entry| %.3f'
          % (n_vp, err.max(), float((err / np.maximum(bound, 1e-30)).max()), np.abs(want).max()))
    assert np.all(err <= bound)
    # without the attended half the entry holds the action half's tables alone
    store2 = features.FeatureStore(table)
    assert store2.gate_rows(dec, attended=False)['attended'] is None


@pytest.mark.parametrize('B', [1, 33, 100])
def test_cell_on_the_location_columns_with_both_rows_against_float64(B):
    """sf_lstm_cell_rows_fwd with x_col0 = F + IMG: gates = xin[:, F+IMG:2F] W_ih[:, F+IMG:2F]^T + h0 W_hh^T + xg + xg2 + b,
    through the path a step takes (0: both rows) and through the product with the cell kernel (1: that kernel has one
    addend, so xg alone -- and both rows there are refused), against float64.  The pre-activations carry the fp32
    product's error: 2.5e-7 * sum |a| |b| on the products plus 2^-23 on the sum of the six terms; sigmoid and tanh have
    slope <= 1 and c1, h1 are sums of products of values in [-1, 1] and c0: the bound below is 4 x (that + 2^-22 (1 +
    |c0|)) for c1 and h1."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import ptr, ws_args
    H, IMG, LOC = synth.FULL.hidden, synth.FULL.img, 128
    F, N = IMG + LOC, 4 * H
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu')
    g.manual_seed(100 + B)
    rn = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    x, h0, c0 = rn(B, 2 * F), rn(B, H) * 0.5, rn(B, H)
    w_ih, w_hh, b_ih, b_hh = rn(N, 2 * F) * 0.05, rn(N, H) * 0.05, rn(N) * 0.1, rn(N) * 0.1
    xg, xg2 = rn(B, N) * 0.5, rn(B, N) * 0.5
    d = lambda t: t.to(dev).contiguous()                              # noqa: E731
    X, H0, C0, WI, WH, BI, BH, XG, XG2 = (d(t) for t in (x, h0, c0, w_ih, w_hh, b_ih, b_hh, xg, xg2))
    f64 = lambda t: t.numpy().astype(np.float64)                      # noqa: E731
    a, wl = f64(x)[:, F + IMG:], f64(w_ih)[:, F + IMG:]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))                          # noqa: E731
    w = _lib.LstmW(WI.data_ptr(), WH.data_ptr(), BI.data_ptr(), BH.data_ptr())
    H1, C1 = torch.full((B, H), float('nan'), device=dev), torch.full((B, H), float('nan'), device=dev)

    def cell(path, second):
        return _lib.lib.sf_lstm_cell_rows_fwd(C.byref(w), B, 2 * F, H, ptr(X), 2 * F, F + IMG, ptr(XG), ptr(second), ptr(H0),
                                              ptr(C0), ptr(H1), ptr(C1), None, path, *ws_args(dev))
    assert cell(1, XG2) == _lib.SF_ERR_UNSUPPORTED                  # (nothing was launched)
    for path, second in ((0, XG2), (1, None)):
        pre = a @ wl.T + f64(h0) @ f64(w_hh).T + f64(xg) + (f64(xg2) if second is not None else 0.0) + f64(b_ih) + f64(b_hh)
        perr = 2.5e-7 * (np.abs(a) @ np.abs(wl).T + np.abs(f64(h0)) @ np.abs(f64(w_hh)).T) + 2.0 ** -23 * 6 * np.abs(pre).max()
        i, f, gg, o = sig(pre[:, :H]), sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
        c1 = f * f64(c0) + i * gg
        h1 = o * np.tanh(c1)
        pe = perr.reshape(B, 4, H).max(axis=1)
        bound = 4 * (pe * (1 + np.abs(f64(c0))) + 2.0 ** -22 * (1 + np.abs(f64(c0))))
        H1.fill_(float('nan'))
        C1.fill_(float('nan'))
        _lib.check(cell(path, second), 'sf_lstm_cell_rows_fwd')
        torch.cuda.synchronize()
        ec, eh = np.abs(f64(C1.cpu()) - c1), np.abs(f64(H1.cpu()) - h1)
        print('[cell rows B=%d path %d] c1 max err %.3e (err / bound %.3f), h1 %.3e (%.3f)'
              % (B, path, ec.max(), float((ec / bound).max()), eh.max(), float((eh / bound).max())))
        assert np.all(ec <= bound) and np.all(eh <= bound)


_oracle = {}


def _reference(key, fb, table, enc_w, dec_w):
    """The numpy oracle's rollout of one case: computed once, shared."""
    if key not in _oracle:
        seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, 80, reverse=True)
        loc = np_env.static_loc_embeddings()
        _oracle[key] = np_model.follower_rollout(
            enc_w, dec_w, seq, lens, mask, S, lambda t: np_env.dense_follower_step(table, loc, fb, t), fb.target, key[1],
            2176, early_exit=False)
    return _oracle[key]


def _pair(enc, dec, store, batch, feedback):
    """The same rollout with the attended rows off and on, `gate_rows` on in both."""
    from speaker_follower_amd import _lib, follower
    off = follower.FollowerEngine(enc, dec, store)
    off.project, off.gate_rows_attended = True, False
    su = _run(off, batch, S, feedback)
    assert su.projected and su.gate_rows and not su.gate_rows_attended
    on = follower.FollowerEngine(enc, dec, store)
    on.project = True
    steps0 = _lib.lib.sf_gate_rows_attended_steps()
    sg = _run(on, batch, S, feedback)
    assert sg.projected and sg.gate_rows and sg.gate_rows_attended
    assert _lib.lib.sf_gate_rows_attended_steps() - steps0 == S - 1
    return su, sg


def _compare(tag, su, sg):
    lu, lg = su.logits.cpu().numpy(), sg.logits.cpu().numpy()
    fin = np.isfinite(lu)
    assert np.array_equal(fin, np.isfinite(lg))
    scale = float(np.abs(lu[fin]).max())
    d = float(np.abs(lg[fin] - lu[fin]).max())
    dl = abs(float(sg.loss_buf) - float(su.loss_buf))
    av_u, av_g = su.tape['alpha_v'], sg.tape['alpha_v']
    da = float((av_g[2:] - av_u[2:]).abs().max()) if av_u.shape[0] > 2 else 0.0
    print('[attended rows, %s] max |logit| %.2f, on vs off %.2e (bound %.2e), later alpha_v %.2e, loss %.3e'
          % (tag, scale, d, 3e-5 * max(scale, 1.0), da, dl))
    assert torch.equal(sg.actions, su.actions)
    assert 0 < d <= 3e-5 * max(scale, 1.0)                        # (> 0: the gate-space partials and the short product ran)
    assert torch.equal(sg.logits[0], su.logits[0])               # step 0 ...
    assert torch.equal(av_g[:2], av_u[:2])                       # ... and alpha_v of step 1: formed before anything differs
    assert torch.allclose(av_g[2:], av_u[2:], rtol=1e-4, atol=1e-6)
    assert dl <= 1e-5 * max(1.0, abs(float(su.loss_buf)))
    return lg


@pytest.mark.parametrize('feedback', ['argmax', 'teacher', 'sample'])
@pytest.mark.parametrize('B', [1, 16, 100])
def test_chain_on_against_off_and_the_oracle(B, feedback):
    from speaker_follower_amd import features, follower
    enc, dec, enc_w, dec_w = _models()
    fb = _edge_batch(B, S)
    table = synth.feature_table(5, NVP)
    store = features.FeatureStore(table)
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    su, sg = _pair(enc, dec, store, batch, feedback)
    lg = _compare('%s B=%d' % (feedback, B), su, sg)
    if feedback == 'sample':                                        # (the reference's torch RNG stream cannot be reproduced)
        return
    ref = _reference((B, feedback), fb, table, enc_w, dec_w)
    n = len(ref['logits'])
    assert np.array_equal(sg.actions.cpu().numpy()[:n], ref['actions'])
    for t in range(n):
        a = ref['logits'][t].shape[1]
        ok = np.isfinite(ref['logits'][t])
        assert float(np.abs(lg[t][:, :a][ok] - ref['logits'][t][ok]).max()) <= 1e-4


@pytest.mark.parametrize('feedback', ['argmax', 'teacher', 'sample'])
def test_padded_sample_yields_zero_rows(feedback):
    """vp < 0 marks a padded sample (an all-zero panorama): its attended feature is zero, in gate space too.  Rows 1 and 5
    are padded from step 1 on; on against off under the bounds of every case, and what launch (2) merged for the padded
    rows is exactly zero: their tape holds zeros in the location columns of xin, their weights are uniform (1 / V, every
    score being 0), and the `xg_f` rows themselves are zero.  Those are read where episode_gate_rows carves them: the
    front of the stream's workspace holds xg_next[0], xg_next[1], xg_f[0], xg_f[1], each B * 4H floats rounded up to 64;
    step t leaves its rows in buffer t & 1, and nothing writes there behind the last step."""
    from speaker_follower_amd import features, follower, runtime
    enc, dec, _, _ = _models()
    B = 16
    fb = _edge_batch(B, S)
    fb.vp[1:, 1] = -1
    fb.vp[1:, 5] = -1
    store = features.FeatureStore(synth.feature_table(5, NVP))
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    su, sg = _pair(enc, dec, store, batch, feedback)
    _compare('%s padded' % feedback, su, sg)
    F, IMG = store.F, store.IMG
    V = store.V
    for st in (su, sg):
        assert float(st.tape['xin'][1:S, [1, 5], F + IMG:].abs().max()) == 0.0
        # exp(0 - 0) * (1 / sum of V ones) in fp32 against 1 / V: one division and one product, 4 x 2^-24 relative
        assert float(st.tape['alpha_v'][1:S, [1, 5]].sub(1.0 / V).abs().max()) <= 4 * 2.0 ** -24 / V
    # (the rollout with the rows on ran last: its rows are what the workspace holds)
    H4 = 4 * dec.hidden_size
    row = (B * H4 + 63) // 64 * 64
    ws = runtime.workspace(torch.device('cuda', torch.cuda.current_device())).view(torch.float32)
    live = [b for b in range(B) if b not in (1, 5)]
    for k in (0, 1):                                                # step k left buffer k for step k + 1, padded there
        xg_f = ws[(2 + k) * row:(2 + k) * row + B * H4].reshape(B, H4)
        assert float(xg_f[[1, 5]].abs().max()) == 0.0
        assert bool((xg_f[live].abs().amax(dim=1) > 0).all())       # (it IS the buffer: every live sample's row is there)


def _smallest_v():
    """The smallest V the projected chain accepts at the full dimensions (B = 16, L = 80, A = 14)."""
    from speaker_follower_amd import _lib
    d = synth.FULL
    for V in range(1, 37):
        if _lib.lib.sf_projected_supported(16, d.hidden, 80, 14, V, d.img, 128):
            return V
    raise AssertionError('no V is supported')


@pytest.mark.parametrize('feedback', ['argmax', 'teacher', 'sample'])
def test_smallest_view_count_leaves_the_last_group_partly_empty(feedback):
    """A sample is three groups of 12 views: at the smallest V the chain takes, groups lie partly or wholly beyond V.  The
    store, the location table and the batch are built for that V."""
    from speaker_follower_amd import features, follower
    enc, dec, _, _ = _models()
    V = _smallest_v()
    assert V < 36 and V % 12 != 0 or V < 12, V
    B = 16
    fb = _edge_batch(B, S)
    fb.view[:] = np.minimum(fb.view, V - 1)
    fb.cand_view[:] = np.minimum(fb.cand_view, V - 1)
    table = synth.feature_table(5, NVP)[:, :V].copy()
    store = features.FeatureStore(table)
    assert store.V == V
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    su, sg = _pair(enc, dec, store, batch, feedback)
    _compare('%s V=%d' % (feedback, V), su, sg)


def _world(B=16):
    from speaker_follower_amd import features, follower
    store = features.FeatureStore(synth.feature_table(5, NVP))
    return store, follower.DeviceFollowerBatch.from_synth(_edge_batch(B, S))


def test_capture_replays_bit_equal_and_follows_weight_ih_in_place():
    from speaker_follower_amd import follower
    enc, dec, _, _ = full_size_models(80)                           # (its weights are changed below: not the shared ones)
    store, batch = _world()
    eng = follower.FollowerEngine(enc, dec, store)
    replay, gst = eng.capture(batch, S, 'argmax')
    assert gst.projected and gst.gate_rows and gst.gate_rows_attended
    hit = store.gate_rows(dec, build=False)
    assert hit['builds'] == 1 and hit['attended'] is not None
    outs = []
    for _ in range(3):                                              # replayed three times: bit-equal
        replay()
        torch.cuda.synchronize()
        outs.append((gst.logits.clone(), gst.actions.clone(), gst.h.clone(), gst.c.clone()))
    assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
    ref = _run(follower.FollowerEngine(enc, dec, store), batch, S)  # an eager rollout on the same store: the same bits
    assert ref.gate_rows_attended and all(torch.equal(a, b) for a, b in zip(outs[0], (ref.logits, ref.actions, ref.h, ref.c)))
    assert store.gate_rows(dec, build=False)['builds'] == 1
    # an in-place change of weight_ih refreshes BOTH tables in place, ahead of the replay
    ptrs = [b.data_ptr() for b in hit['bufs']] + [hit['attended']['buf'].data_ptr()]
    gf0 = hit['attended']['buf'][:4].clone()
    with torch.no_grad():
        dec.lstm.weight_ih.mul_(1.25)
    replay()
    torch.cuda.synchronize()
    hit = store.gate_rows(dec, build=False)
    assert hit['builds'] == 2
    assert [b.data_ptr() for b in hit['bufs']] + [hit['attended']['buf'].data_ptr()] == ptrs
    assert torch.allclose(hit['attended']['buf'][:4], gf0 * 1.25, rtol=1e-5, atol=1e-6)
    ref2 = _run(follower.FollowerEngine(enc, dec, store), batch, S)
    assert ref2.gate_rows_attended and torch.equal(gst.logits, ref2.logits) and not torch.equal(gst.logits, outs[0][0])
    # ... and the chain without the attended rows agrees with the refreshed tables
    off = follower.FollowerEngine(enc, dec, store)
    off.gate_rows_attended = False
    ref3 = _run(off, batch, S)
    assert ref3.gate_rows and not ref3.gate_rows_attended and torch.equal(ref3.actions, ref2.actions)
    fin = torch.isfinite(ref3.logits)
    assert float((ref3.logits[fin] - ref2.logits[fin]).abs().max()) <= 3e-5 * max(1.0, float(ref3.logits[fin].abs().max()))


def test_capture_with_the_switch_off_survives_refresh_and_another_engines_table():
    """`gate_rows_attended = False` follows the same rules: a rollout captured that way is refreshed in place when
    `weight_ih` changes -- the action half's tables alone; the refresh never adds the table the engine declined -- and
    replays without WeightsMoved, again and again.  When ANOTHER engine then builds the attended half's table into the
    same entry (the action half's pointers stay), the first graph, which never reads it, still replays; and a rollout
    captured with the table follows the next change of `weight_ih` with both tables in place."""
    from speaker_follower_amd import follower
    enc, dec, _, _ = full_size_models(81)                           # (its weights are changed below: not the shared ones)
    store, batch = _world()
    a = follower.FollowerEngine(enc, dec, store)
    a.gate_rows_attended = False
    replay_a, sa = a.capture(batch, S, 'argmax')
    replay_a()
    torch.cuda.synchronize()
    assert sa.projected and sa.gate_rows and not sa.gate_rows_attended
    hit = store.gate_rows(dec, build=False, attended=False)
    assert hit['builds'] == 1 and hit['attended'] is None
    ptrs = [b.data_ptr() for b in hit['bufs']]
    first = sa.logits.clone()
    for k in (2, 3):                                                # two updates: the second replay must not raise either
        with torch.no_grad():
            dec.lstm.weight_ih.mul_(1.25)
        replay_a()
        torch.cuda.synchronize()
        hit = store.gate_rows(dec, build=False, attended=False)
        assert hit['builds'] == k and hit['attended'] is None and [b.data_ptr() for b in hit['bufs']] == ptrs
        assert store.gate_rows(dec, build=False)['attended'] is None    # (asking with the default does not add it either)
    assert not torch.equal(sa.logits, first)
    eager = follower.FollowerEngine(enc, dec, store)
    eager.gate_rows_attended = False
    ref = _run(eager, batch, S)
    assert ref.gate_rows and not ref.gate_rows_attended and torch.equal(ref.logits, sa.logits)
    # another engine builds the attended half's table into the entry: one more build, the same GU / GL
    b = follower.FollowerEngine(enc, dec, store)
    replay_b, sb = b.capture(batch, S, 'argmax')
    replay_b()
    torch.cuda.synchronize()
    hit = store.gate_rows(dec, build=False)
    assert sb.gate_rows_attended and hit['builds'] == 4 and hit['attended'] is not None
    assert [x.data_ptr() for x in hit['bufs']] == ptrs
    want = sa.logits.clone()
    replay_a()                                                      # (its graph never reads GF: no WeightsMoved)
    torch.cuda.synchronize()
    assert torch.equal(sa.logits, want)
    gf = hit['attended']['buf'].data_ptr()
    with torch.no_grad():
        dec.lstm.weight_ih.mul_(0.8)
    replay_b()
    replay_a()
    torch.cuda.synchronize()
    hit = store.gate_rows(dec, build=False)
    assert hit['builds'] == 5 and hit['attended']['buf'].data_ptr() == gf and [x.data_ptr() for x in hit['bufs']] == ptrs
    fin = torch.isfinite(sa.logits)
    assert torch.equal(sa.actions, sb.actions)
    assert 0 < float((sa.logits[fin] - sb.logits[fin]).abs().max()) <= 3e-5 * max(1.0, float(sa.logits[fin].abs().max()))


@pytest.mark.parametrize('case', ['gate_rows False', 'project False', 'bf16', 'late partials'])
def test_declining_cases_reproduce_the_bits_with_the_attended_rows_off(case):
    """Every case that declines launches what it launched without the table: bit for bit the rollout of an engine with
    `gate_rows_attended = False` under the same settings, and the step counter stands still.  The tables exist (another
    engine built them), so it is the library and the engine's policy that decline, not their absence.  (The new switch
    itself: test_library_switch_off_declines_with_the_table_registered.  An H for which the partials do not take rows of
    4H + LOC floats lies above 512, where the projected chain does not run at all: tests/test_gate_rows_attended_host.py
    holds the rule.)"""
    from speaker_follower_amd import _lib, follower
    enc, dec, _, _ = _models()
    store, batch = _world()
    builder = follower.FollowerEngine(enc, dec, store)
    builder.project = True
    assert _run(builder, batch, S).gate_rows_attended and store.gate_rows(dec, build=False)['attended'] is not None

    def settings(eng):
        eng.project = True
        if case == 'gate_rows False':
            eng.gate_rows = False
        elif case == 'project False':
            eng.project = False
        elif case == 'bf16':
            eng.gate_weights = 'bf16'

    out = {}
    for att in (True, False):
        eng = follower.FollowerEngine(enc, dec, store)
        settings(eng)
        eng.gate_rows_attended = att
        steps0 = _lib.lib.sf_gate_rows_attended_steps()
        if case == 'late partials':
            _lib.lib.sf_debug_projected_partials_late(1)
            try:
                st = _run(eng, batch, S)
            finally:
                _lib.lib.sf_debug_projected_partials_late(0)
        else:
            st = _run(eng, batch, S)
        assert not st.gate_rows_attended and _lib.lib.sf_gate_rows_attended_steps() == steps0
        assert bool(st.gate_rows) == (case == 'late partials')
        out[att] = (st.logits.clone(), st.actions.clone(), st.h.clone(), st.c.clone(), st.tape['alpha_v'].clone())
    assert all(torch.equal(a, b) for a, b in zip(out[True], out[False]))


def test_library_switch_off_declines_with_the_table_registered():
    """sf_gate_rows_attended_use(0) around an engine that asks for the attended rows: the episode runs on the action half's
    rows alone, bit for bit the engine with `gate_rows_attended = False`."""
    from speaker_follower_amd import _lib, follower
    enc, dec, _, _ = _models()
    store, batch = _world()
    builder = follower.FollowerEngine(enc, dec, store)
    builder.project = True
    assert _run(builder, batch, S).gate_rows_attended
    off = follower.FollowerEngine(enc, dec, store)
    off.gate_rows_attended = False
    want = _run(off, batch, S)
    eng = follower.FollowerEngine(enc, dec, store)
    real = follower.gate_rows_attended_pass
    follower.gate_rows_attended_pass = lambda on: real(False)       # (the engine's own pass forced off: the library declines)
    try:
        steps0 = _lib.lib.sf_gate_rows_attended_steps()
        got = _run(eng, batch, S)
    finally:
        follower.gate_rows_attended_pass = real
    assert got.gate_rows and not got.gate_rows_attended and _lib.lib.sf_gate_rows_attended_steps() == steps0
    assert torch.equal(got.logits, want.logits) and torch.equal(got.h, want.h) and torch.equal(got.c, want.c)
