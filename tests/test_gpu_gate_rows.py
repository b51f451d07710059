"""GPU: GATE-SPACE ROWS for the action half of the decoder LSTM's input (include/sf_hip.h: sf_gate_rows_build; csrc/sf_api_follower.hip:
sf_follower_episode_fwd) -- launch (2) of the projected chain leaves the chosen action's row as GU[vp V + view] +
sum_k sincos_k GL[k], and the next step's gate product runs over K = F + H instead of 2 F + H.

Checked here, at the full model dimensions with peaky weights and tiny feature tables:
  * GU and GL, every entry, against float64 numpy formed from the same fp32 weights (one chunk and several), and a few rows at
    both ends of a table whose last GU row starts beyond 2^31 bytes;
  * the chain against the projected chain with the rows switched off and against the numpy oracle of the reference, for
    argmax, teacher and sample feedback, on batches that hold rows stopping at step 0, the last candidate slot chosen,
    candidate views 0 and V - 1 and the first and last table row, at B = 1, 16 and 100;
  * the policy: what builds, what only uses, the in-place refresh behind a captured rollout, the cases that decline."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402
from oracle import np_env, np_model                                   # noqa: E402
from tests.follower_models import full_size_models                    # noqa: E402

NVP = 24
_cache = {}


def _models(seed=77):
    if seed not in _cache:
        _cache[seed] = full_size_models(seed)
    return _cache[seed]


def _edge_batch(B, S=3, nvp=NVP):
    """synth.follower_batch with the edges of the index space written in.  Per step t one row `lo` whose only candidate is
    stop (a_num = 1) and one row `hi` with every slot in use (a_num = A), at views 0 / V - 1 and table rows 0 / nvp - 1,
    candidate views 0 and V - 1 in slots 1 and A - 1.  The TEACHER's targets: row `hi` takes the last slot (a* = a_num - 1,
    candidate view V - 1) at even t and slot 1 (view 0) at odd t; every fifth row stops at step 0; every other live row
    takes its last candidate -- so that, under teacher feedback, each of those rows is what the next step's cell reads."""
    fb = synth.follower_batch(seed=11 + B, batch=B, steps=S, n_viewpoints=nvp, min_len=2, max_len=12)
    A, V = fb.a_max, synth.FULL.views
    for t in range(S):
        lo, hi = t % B, (B - 1 - t) % B
        if B > 1 or t == S - 1:                                     # (B = 1: the full list first, stop-only at the end)
            fb.a_num[t, lo] = 1
        if hi != lo or t == 0:
            fb.a_num[t, hi] = A
        fb.view[t, lo], fb.vp[t, lo] = (0, 0) if t % 2 == 0 else (V - 1, nvp - 1)
        fb.view[t, hi], fb.vp[t, hi] = (V - 1, nvp - 1) if t % 2 == 0 else (0, 0)
        fb.cand_view[t, hi, 1], fb.cand_view[t, hi, A - 1] = 0, V - 1
        fb.target[t] = fb.a_num[t] - 1
        if fb.a_num[t, hi] == A and t % 2 == 1:
            fb.target[t, hi] = 1
    if B > 1:
        fb.target[0, 2::5] = 0                                      # rows that choose stop at step 0
    return fb


def _w_ih64(dec_w):
    return np.asarray(dec_w['lstm.weight_ih'], np.float64)          # [4H, 2F]


@pytest.mark.parametrize('n_vp,chunk', [(1, 0), (3, 0), (15, 0), (30, 512), (5, 64)])
def test_tables_match_float64_numpy(n_vp, chunk):
    """Every entry of GU and GL within 2.5e-7 * sum |a| |b| of the float64 product of the same fp32 weights (the bound
    tests/test_gpu_projected.py holds PV / PA to).  n_vp = 15 (540 rows) is the smallest table whose product is the
    many-row kernel's; chunk > 0 (sf_debug_projected_chunk_rows) builds in several chunks -- 512 + 512 + 56 rows on the
    many-row kernel, 64 + 64 + 52 on the small ones: the row offsets between chunks."""
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
    gu, gl = (b.cpu().numpy().astype(np.float64) for b in hit['bufs'])
    H, IMG, LOC = synth.FULL.hidden, synth.FULL.img, 128
    w = _w_ih64(dec_w)
    x = table.reshape(-1, IMG).astype(np.float64)
    assert gu.shape == (n_vp * 36, 4 * H) and gl.shape == (4, 4 * H)

    def check(name, got, rows, wt):
        want, bound = rows @ wt.T, 2.5e-7 * (np.abs(rows) @ np.abs(wt).T)
        err = np.abs(got - want)
        print('[%s n_vp=%d] max err %.3e, max err / bound %.3f, max |entry| %.3f'
              % (name, n_vp, err.max(), float((err / np.maximum(bound, 1e-30)).max()), np.abs(want).max()))
        assert np.all(err <= bound)

    check('GU', gu, x, w[:, :IMG])
    onehot = np.zeros((4, LOC))
    for q in range(4):
        onehot[q, q * (LOC // 4):(q + 1) * (LOC // 4)] = 1.0
    check('GL', gl, onehot, w[:, IMG:IMG + LOC])
    np.testing.assert_allclose(gl, features.gate_loc_groups(w[:, IMG:IMG + LOC]), rtol=0, atol=1e-5)


def test_rows_beyond_two_to_the_31_bytes():
    """7 282 viewpoints: the smallest table whose last GU row (row 262 151 of 8 KB) starts beyond 2^31 bytes.  The table is
    generated on the device; a few rows at both ends against float64."""
    from speaker_follower_amd import features
    enc, dec, _, dec_w = _models()
    n_vp, V, IMG, H = 7282, 36, synth.FULL.img, synth.FULL.hidden
    assert (n_vp * V - 1) * 4 * H * 4 > 2 ** 31 > ((n_vp - 1) * V - 1) * 4 * H * 4
    g = torch.Generator(device='cuda')
    g.manual_seed(3)
    table = torch.rand(n_vp, V, IMG, device='cuda', generator=g)
    store = features.FeatureStore(table)
    hit = store.gate_rows(dec)
    torch.cuda.synchronize()
    gu = hit['bufs'][0]
    rows = [0, 1, 35, 36, 16383, 16384, n_vp * V - 37, n_vp * V - 2, n_vp * V - 1]
    idx = torch.tensor(rows, device='cuda')
    got = gu[idx].cpu().numpy().astype(np.float64)
    x = store.table.reshape(-1, IMG)[idx].cpu().numpy().astype(np.float64)
    w = _w_ih64(dec_w)[:, :IMG]
    err, bound = np.abs(got - x @ w.T), 2.5e-7 * (np.abs(x) @ np.abs(w).T)
    print('[GU 2^31] max err %.3e, max err / bound %.3f' % (err.max(), float((err / bound).max())))
    assert np.all(err <= bound)
    del hit, gu, store, table
    torch.cuda.empty_cache()


def _run(eng, batch, S, feedback='argmax'):
    with torch.no_grad():
        st = eng.rollout(batch, S, feedback, train=False)
    torch.cuda.synchronize()
    return st


_oracle = {}


def _reference(B, S, feedback, fb, table, enc_w, dec_w):
    """The numpy oracle's rollout of (B, feedback): computed once, shared."""
    if (B, feedback) not in _oracle:
        seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, 80, reverse=True)
        loc = np_env.static_loc_embeddings()
        _oracle[(B, feedback)] = np_model.follower_rollout(
            enc_w, dec_w, seq, lens, mask, S, lambda t: np_env.dense_follower_step(table, loc, fb, t), fb.target, feedback,
            2176, early_exit=False)
    return _oracle[(B, feedback)]


@pytest.mark.parametrize('feedback', ['argmax', 'teacher', 'sample'])
@pytest.mark.parametrize('B', [1, 16, 100])
def test_chain_equals_the_projected_chain_without_gate_rows_and_the_oracle(B, feedback):
    from speaker_follower_amd import features, follower
    enc, dec, enc_w, dec_w = _models()
    S = 3
    fb = _edge_batch(B, S)
    table = synth.feature_table(5, NVP)
    store = features.FeatureStore(table)
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    off = follower.FollowerEngine(enc, dec, store)
    off.project, off.gate_rows = True, False
    su = _run(off, batch, S, feedback)
    assert su.projected and not su.gate_rows and store.gate_rows(dec, build=False) is None
    on = follower.FollowerEngine(enc, dec, store)
    on.project = True
    sg = _run(on, batch, S, feedback)
    assert sg.projected and sg.gate_rows
    lu, lg = su.logits.cpu().numpy(), sg.logits.cpu().numpy()
    au, ag = su.actions.cpu().numpy(), sg.actions.cpu().numpy()
    fin = np.isfinite(lu)
    assert np.array_equal(fin, np.isfinite(lg))
    scale = float(np.abs(lu[fin]).max())
    d = float(np.abs(lg[fin] - lu[fin]).max())
    dh = float((sg.h - su.h).abs().max())
    dl = abs(float(sg.loss_buf) - float(su.loss_buf))
    print('[gate rows, %s] B=%d: max |logit| %.2f, with vs without %.2e, h %.2e, loss %.3e' % (feedback, B, scale, d, dh, dl))
    assert 0 < d <= 3e-5 * max(scale, 1.0)                        # (> 0: the short product and the gathered row really ran)
    assert np.array_equal(ag, au)
    assert torch.equal(sg.logits[0], su.logits[0])               # step 0 keeps the full product: bit for bit
    assert dl <= 1e-5 * max(1.0, abs(float(su.loss_buf)))
    # the raw row is still written: the tape's xin is what it was, bit for bit (the actions are equal)
    F = store.F
    assert torch.equal(sg.tape['xin'][1:S, :, :F], su.tape['xin'][1:S, :, :F])
    if feedback == 'teacher':
        # the edges really are what the cells read: rows that stopped at step 0, the last slot, slot 1
        A = fb.a_max
        hi0 = (B - 1) % B
        assert ag[0, hi0] == A - 1 and (B == 1 or np.all(ag[0, 2::5] == 0))
        assert B == 1 or ag[1, (B - 2) % B] == 1
    if feedback == 'sample':                                        # (the reference's torch RNG stream cannot be reproduced)
        return
    ref = _reference(B, S, feedback, fb, table, enc_w, dec_w)
    n = len(ref['logits'])
    assert np.array_equal(ag[:n], ref['actions'])
    for t in range(n):
        a = ref['logits'][t].shape[1]
        ok = np.isfinite(ref['logits'][t])
        assert float(np.abs(lg[t][:, :a][ok] - ref['logits'][t][ok]).max()) <= 1e-4


def _world(B=16, S=3):
    from speaker_follower_amd import features, follower
    store = features.FeatureStore(synth.feature_table(5, NVP))
    return store, follower.DeviceFollowerBatch.from_synth(_edge_batch(B, S))


def test_policy_capture_builds_eager_uses_and_replay_follows_weight_ih():
    from speaker_follower_amd import _lib, follower
    enc, dec, _, _ = full_size_models(78)                           # (its weights are changed below: not the shared ones)
    S = 3
    # an eager rollout under 'auto' builds nothing -- not with projected tables at hand either
    store, batch = _world()
    first = follower.FollowerEngine(enc, dec, store)
    first.gate_rows = False
    replay_off, gst_off = first.capture(batch, S, 'argmax')         # (the projected tables alone)
    replay_off()
    torch.cuda.synchronize()
    assert gst_off.projected and not gst_off.gate_rows and store.gate_rows(dec, build=False) is None
    eager = _run(follower.FollowerEngine(enc, dec, store), batch, S)
    assert eager.projected and not eager.gate_rows and store.gate_rows(dec, build=False) is None
    assert torch.equal(eager.logits, gst_off.logits)
    # capture() builds them
    store, batch = _world()
    eng = follower.FollowerEngine(enc, dec, store)
    replay, gst = eng.capture(batch, S, 'argmax')
    assert gst.projected and gst.gate_rows and store.gate_rows(dec, build=False)['builds'] == 1
    outs = []
    for _ in range(3):                                              # replayed three times: bit-equal
        replay()
        torch.cuda.synchronize()
        outs.append((gst.logits.clone(), gst.actions.clone(), gst.h.clone()))
    assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
    a = outs[0][0]
    # an eager rollout on that store launches what the replay does: the short gate product behind step 0
    fresh = follower.FollowerEngine(enc, dec, store)
    with torch.no_grad():
        fresh.rollout(batch, S, 'argmax', train=False)
        torch.cuda.synchronize()
        steps0 = _lib.lib.sf_gate_rows_steps()
        ref = fresh.rollout(batch, S, 'argmax', train=False)
        torch.cuda.synchronize()
    assert ref.gate_rows and _lib.lib.sf_gate_rows_steps() - steps0 == S - 1
    assert torch.equal(a, ref.logits) and torch.equal(gst.actions, ref.actions)
    assert store.gate_rows(dec, build=False)['builds'] == 1
    # an in-place change of weight_ih: refreshed in place ahead of the replay
    ptrs = [b.data_ptr() for b in store.gate_rows(dec, build=False)['bufs']]
    with torch.no_grad():
        dec.lstm.weight_ih.mul_(1.25)
    replay()
    torch.cuda.synchronize()
    hit = store.gate_rows(dec, build=False)
    assert hit['builds'] == 2 and [b.data_ptr() for b in hit['bufs']] == ptrs
    ref2 = _run(follower.FollowerEngine(enc, dec, store), batch, S)
    assert ref2.gate_rows and torch.equal(gst.logits, ref2.logits) and not torch.equal(gst.logits, a)
    # ... and the full product agrees with the refreshed tables
    off = follower.FollowerEngine(enc, dec, store)
    off.gate_rows = False
    ref3 = _run(off, batch, S)
    assert ref3.projected and not ref3.gate_rows and torch.equal(ref3.actions, ref2.actions)
    fin = torch.isfinite(ref3.logits)
    assert float((ref3.logits[fin] - ref2.logits[fin]).abs().max()) <= 3e-5 * max(1.0, float(ref3.logits[fin].abs().max()))
    # a re-allocated weight cannot be patched into the graph
    w = dec.lstm.weight_ih
    w.data = w.data.clone()
    with pytest.raises(follower.WeightsMoved):
        replay()


@pytest.mark.parametrize('case', ['bf16', 'project False'])
def test_declining_cases_reproduce_the_bits_without_gate_rows(case):
    """`gate_weights = 'bf16'` (the packed images cover the whole W_ih) and `project = False`: no gate rows are built or
    used, and the rollout is bit for bit the one with `gate_rows = False`."""
    from speaker_follower_amd import follower
    enc, dec, _, _ = _models()
    S = 3
    store, batch = _world()
    out = {}
    for rows in (True, False):
        eng = follower.FollowerEngine(enc, dec, store)
        eng.gate_rows = rows
        if case == 'bf16':
            eng.project, eng.gate_weights = True, 'bf16'
        else:
            eng.project = False
        st = _run(eng, batch, S)
        assert not st.gate_rows and bool(st.projected) == (case == 'bf16')
        out[rows] = (st.logits.clone(), st.actions.clone(), st.h.clone(), st.c.clone())
    assert all(torch.equal(a, b) for a, b in zip(out[True], out[False]))
    assert store.gate_rows(dec, build=False) is None                # (nothing was built for a rollout that cannot use it)
    # ... and with the tables at hand the library itself declines for the packed pair
    if case == 'bf16':
        on = follower.FollowerEngine(enc, dec, store)
        on.project = True
        assert _run(on, batch, S).gate_rows and store.gate_rows(dec, build=False) is not None
        from speaker_follower_amd import _lib
        eng = follower.FollowerEngine(enc, dec, store)
        eng.project, eng.gate_weights = True, 'bf16'
        eng._gate_rows_tables = lambda projected, train: store.gate_rows(dec, build=False)   # (the engine's own check bypassed)
        steps0 = _lib.lib.sf_gate_rows_steps()
        st = _run(eng, batch, S)
        assert _lib.lib.sf_gate_rows_steps() == steps0 and not st.gate_rows
        assert all(torch.equal(a, b) for a, b in zip((st.logits, st.actions, st.h, st.c), out[False]))
