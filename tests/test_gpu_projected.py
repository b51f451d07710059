"""GPU: the PROJECTED decode chain (include/sf_hip.h: sf_projected_build; csrc/sf_api_follower.hip: tail_proj) -- scores of the
panorama and of the candidates taken from feature-table rows carried through the folded query / scoring matrices once per
(table, weights), two dependent launches per decode step behind the cell instead of four.

Checked here, at the full model dimensions with peaky weights (flat ones give logits near 0 and prove nothing) and tiny
feature tables:
  * the four tables, every entry, against float64 numpy formed from the same fp32 weights;
  * the chain against the four-launch folded chain of the same build and against the numpy oracle of the reference, on
    batches that hold a stop-only sample, a full candidate list, view indices 0 and 35 and the first and last table row;
  * the policy (`FollowerEngine.project`), the in-place refresh behind a captured rollout, and every case that declines."""
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
    """synth.follower_batch with the edges of the index space written in: a sample whose only candidate is `stop`
    (a_num = 1), one with every candidate slot in use (a_num = A), agent and candidate view indices 0 and 35, the first
    and the last row of the feature table."""
    fb = synth.follower_batch(seed=11 + B, batch=B, steps=S, n_viewpoints=nvp, min_len=2, max_len=12)
    A, V = fb.a_max, synth.FULL.views
    for t in range(S):
        lo, hi = t % B, (B - 1 - t) % B
        if B > 1 or t == S - 1:                                     # (B = 1: the full list first, stop-only at the end)
            fb.a_num[t, lo] = 1
            if fb.target[t, lo] > 0:
                fb.target[t, lo] = 0
        if hi != lo or t == 0:
            fb.a_num[t, hi] = A
        fb.view[t, lo], fb.vp[t, lo] = (0, 0) if t % 2 == 0 else (V - 1, nvp - 1)
        fb.view[t, hi], fb.vp[t, hi] = (V - 1, nvp - 1) if t % 2 == 0 else (0, 0)
        fb.cand_view[t, hi, 1], fb.cand_view[t, hi, A - 1] = 0, V - 1
    return fb


def _fold64(dec_w):
    """M_v, c_v, M_a, c_a, m, c0 of sf_decoder_fold in float64 from the fp32 weights."""
    g = lambda k: np.asarray(dec_w[k], np.float64)   # noqa: E731
    vh, vb, vv = g('visual_attention_layer.linear_in_h.weight'), g('visual_attention_layer.linear_in_h.bias'), \
        g('visual_attention_layer.linear_in_v.weight')
    ah, ab, aa, aab = g('decoder2action.linear_in_h.weight'), g('decoder2action.linear_in_h.bias'), \
        g('decoder2action.linear_in_a.weight'), g('decoder2action.linear_in_a.bias')
    wo, bo = g('decoder2action.linear_out.weight').reshape(-1), g('decoder2action.linear_out.bias').reshape(-1)
    m_v, c_v = vv.T @ vh, vv.T @ vb                                    # [F,H], [F]
    m_a, c_a = (aa.T * wo) @ ah, aa.T @ (wo * ab)                      # [F,H], [F]
    m, c0 = (wo * aab) @ ah, float((wo * ab) @ aab + bo[0])
    # the same with every factor replaced by its magnitude: what bounds the rounding of the chained products
    n_v, d_v = np.abs(vv).T @ np.abs(vh), np.abs(vv).T @ np.abs(vb)
    n_a, d_a = (np.abs(aa).T * np.abs(wo)) @ np.abs(ah), np.abs(aa).T @ np.abs(wo * ab)
    n_m, d_c0 = np.abs(wo * aab) @ np.abs(ah), float(np.abs(wo * ab) @ np.abs(aab) + abs(bo[0]))
    return dict(m_v=m_v, c_v=c_v, m_a=m_a, c_a=c_a, m=m, c0=c0, n_v=n_v, d_v=d_v, n_a=n_a, d_a=d_a, n_m=n_m, d_c0=d_c0)


@pytest.mark.parametrize('n_vp,chunk', [(1, 0), (3, 0), (15, 0), (30, 512), (5, 64)])
def test_tables_match_float64_numpy(n_vp, chunk):
    """Every entry of PV, PA, LV and LA within 2.5e-7 * sum |a| |b| of the float64 product of the same fp32 weights (the
    bound tests/test_gpu_gate_bf16.py and the GEMM edge tests hold the split kernels to); the padding columns are zero.
    n_vp = 15 (540 rows) is the smallest table whose product is the many-row kernel's (M >= 512: the one that builds
    the real tables, with its N = 516 tile tail); chunk > 0 (sf_debug_projected_chunk_rows) builds in several chunks --
    512 + 512 + 56 rows on the many-row kernel, 64 + 64 + 52 on the small ones: the row offsets between chunks."""
    from speaker_follower_amd import _lib, features
    enc, dec, _, dec_w = _models()
    table = synth.feature_table(5, n_vp)
    store = features.FeatureStore(table)
    _lib.lib.sf_debug_projected_chunk_rows(chunk)
    try:
        hit = store.projected(dec)
        torch.cuda.synchronize()
    finally:
        _lib.lib.sf_debug_projected_chunk_rows(0)
    pv, pa, lv, la = (b.cpu().numpy().astype(np.float64) for b in hit['bufs'])
    f = _fold64(dec_w)
    H, IMG, LOC = synth.FULL.hidden, synth.FULL.img, 128
    x = table.reshape(-1, IMG).astype(np.float64)
    loc = store.loc_table.cpu().numpy().reshape(-1, LOC).astype(np.float64)
    assert pv.shape == (n_vp * 36, H + 4) and la.shape == (5, H + 4) and lv.shape == (36 * 36, H + 4)

    def check(name, got, rows, mat, vec, amat, avec):
        want = np.concatenate((rows @ mat, (rows @ vec)[:, None]), 1)
        bound = 2.5e-7 * np.concatenate((np.abs(rows) @ amat, (np.abs(rows) @ avec)[:, None]), 1)
        err = np.abs(got[:, :H + 1] - want)
        print('[%s n_vp=%d] max err %.3e, max err / bound %.3f, max |entry| %.3f'
              % (name, n_vp, err.max(), float((err / np.maximum(bound, 1e-30)).max()), np.abs(want).max()))
        assert np.all(got[:, H + 1:] == 0)
        assert np.all(err <= bound)

    check('PV', pv, x, f['m_v'][:IMG], f['c_v'][:IMG], f['n_v'][:IMG], f['d_v'][:IMG])
    check('PA', pa, x, f['m_a'][:IMG], f['c_a'][:IMG], f['n_a'][:IMG], f['d_a'][:IMG])
    check('LV', lv, loc, f['m_v'][IMG:], f['c_v'][IMG:], f['n_v'][IMG:], f['d_v'][IMG:])
    # LA's group blocks follow cand_load's layout: a candidate whose sin/cos vector is the g-th unit vector has the
    # location part of features.build_loc_table's layout -- ones over block g -- and LA[g] is that row projected
    g = LOC // 4
    onehot = np.zeros((4, LOC))
    for q in range(4):
        onehot[q, q * g:(q + 1) * g] = 1.0
    check('LA', la[:4], onehot, f['m_a'][IMG:], f['c_a'][IMG:], f['n_a'][IMG:], f['d_a'][IMG:])
    # row 4: the constant row of the scoring fold, [m | c0]
    want4, bound4 = np.concatenate((f['m'], [f['c0']])), 2.5e-7 * np.concatenate((f['n_m'], [f['d_c0']]))
    assert np.all(np.abs(la[4, :H + 1] - want4) <= bound4), float((np.abs(la[4, :H + 1] - want4) / bound4).max())


def test_la_groups_score_like_the_dense_candidate_rows():
    """The same layout seen from the data side: the location part of a dense candidate row (features.cand_sincos through
    sf_gather_candidates) dotted with M_a[IMG:] equals sum_g sc_g LA[g]."""
    from speaker_follower_amd import features
    enc, dec, _, dec_w = _models()
    store = features.FeatureStore(synth.feature_table(5, 2))
    la = store.projected(dec)['bufs'][3].cpu().numpy().astype(np.float64)
    f = _fold64(dec_w)
    H, IMG = synth.FULL.hidden, synth.FULL.img
    sc = features.cand_sincos(np.array([0.3, -2.0, 1.1]), np.array([0.2, -0.4, 0.0]))        # [3,4]
    dev = store.device
    vp = torch.zeros(1, dtype=torch.int32, device=dev)
    cv = torch.tensor([[0, 5, 35, 7]], dtype=torch.int32, device=dev)
    sct = torch.zeros(1, 4, 4, device=dev)
    sct[0, 1:] = torch.from_numpy(sc).to(dev)
    all_u, _ = store.gather_candidates(vp, cv, sct, torch.tensor([4], dtype=torch.int32, device=dev))
    u_loc = all_u[0, 1:, IMG:].cpu().numpy().astype(np.float64)                                # [3,LOC]
    want = u_loc @ f['m_a'][IMG:]
    got = sc.astype(np.float64) @ la[:4, :H]
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


def _run(eng, batch, S):
    with torch.no_grad():
        st = eng.rollout(batch, S, 'argmax', train=False)
    torch.cuda.synchronize()
    return st


def _numbers(st):
    return (st.logits.cpu().numpy().copy(), st.actions.cpu().numpy().copy(), float(st.loss_buf),
            st.tape['alpha_v'].cpu().numpy().copy())


@pytest.mark.parametrize('late', [0, 1])
@pytest.mark.parametrize('B', [1, 16, 17, 37, 100])
def test_projected_chain_equals_the_folded_chain_and_the_oracle(B, late):
    """late: the attention partials in launch (2) (sf_debug_projected_partials_late; the default) or in launch (1)."""
    from speaker_follower_amd import _lib, features, follower
    enc, dec, enc_w, dec_w = _models()
    S = 3
    fb = _edge_batch(B, S)
    table = synth.feature_table(5, NVP)
    store = features.FeatureStore(table)
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    ref_eng = follower.FollowerEngine(enc, dec, store)
    ref_eng.project = False
    su = _run(ref_eng, batch, S)
    assert su.text_folded and not su.projected
    lu, au, lossu, avu = _numbers(su)
    eng = follower.FollowerEngine(enc, dec, store)
    eng.project = True
    _lib.lib.sf_debug_projected_partials_late(late)
    try:
        sp = _run(eng, batch, S)
    finally:
        _lib.lib.sf_debug_projected_partials_late(1)
    assert sp.text_folded and sp.projected
    lp, ap, lossp, avp = _numbers(sp)
    fin = np.isfinite(lu)
    assert np.array_equal(fin, np.isfinite(lp))
    scale = float(np.abs(lu[fin]).max())
    d = float(np.abs(lp[fin] - lu[fin]).max())
    print('[projected%s] B=%d: max |logit| %.2f, projected vs folded %.2e, alpha_v %.2e, loss %.3e'
          % ('' if late else ', partials in launch (1)', B, scale, d, np.abs(avp - avu).max(), abs(lossp - lossu)))
    assert 0 < d <= 3e-5 * max(scale, 1.0)                        # (> 0: the projected kernels really ran)
    assert np.array_equal(ap, au)
    np.testing.assert_allclose(avp.sum(-1), 1.0, atol=1e-5)      # (step 0's too: the head runs on projected rows)
    np.testing.assert_allclose(avp, avu, rtol=1e-4, atol=1e-6)
    assert abs(lossp - lossu) <= 1e-5 * max(1.0, abs(lossu))
    # a stop-only sample scores its one candidate with the constant row alone, everything behind it is masked
    t1 = 0 if B > 1 else S - 1
    assert np.isfinite(lp[t1, 0, 0]) and np.all(np.isinf(lp[t1, 0, 1:]))
    # ... and the reference itself (numpy oracle)
    seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, 80, reverse=True)
    loc = np_env.static_loc_embeddings()
    ref = np_model.follower_rollout(enc_w, dec_w, seq, lens, mask, S,
                                    lambda t: np_env.dense_follower_step(table, loc, fb, t), fb.target, 'argmax', 2176,
                                    early_exit=False)
    n = len(ref['logits'])
    assert np.array_equal(ap[:n], ref['actions'])
    for t in range(n):
        a = ref['logits'][t].shape[1]
        ok = np.isfinite(ref['logits'][t])
        assert float(np.abs(lp[t][:, :a][ok] - ref['logits'][t][ok]).max()) <= 1e-4


def _world(B=16, S=3, seed=77):
    from speaker_follower_amd import features, follower
    enc, dec, _, _ = _models(seed)
    fb = _edge_batch(B, S)
    store = features.FeatureStore(synth.feature_table(5, NVP))
    return enc, dec, store, follower.DeviceFollowerBatch.from_synth(fb)


def test_policy_capture_builds_eager_uses_and_replay_follows_the_weights():
    from speaker_follower_amd import _lib, follower
    enc, dec, _, _ = full_size_models(78)                           # (its weights are changed below: not the shared ones)
    _, _, store, batch = _world()
    S = 3
    eng = follower.FollowerEngine(enc, dec, store)
    assert eng.project == 'auto'
    st0 = _run(eng, batch, S)
    assert st0.text_folded and not st0.projected                    # a fresh store: nothing is built for one rollout
    assert store.projected(dec, build=False) is None
    # ... and a pair that has handed out unprojected results keeps them: the replay is that eager rollout, bit for bit
    replay0, gst0 = eng.capture(batch, S, 'argmax')
    replay0()
    torch.cuda.synchronize()
    assert not gst0.projected and torch.equal(gst0.logits, st0.logits) and store.projected(dec, build=False) is None
    # a fresh store whose first inference rollout is the captured one: the tables are built
    _, _, store, batch = _world()
    eng = follower.FollowerEngine(enc, dec, store)
    replay, gst = eng.capture(batch, S, 'argmax')
    assert gst.projected and store.projected(dec, build=False)['builds'] == 1
    replay()
    torch.cuda.synchronize()
    a = gst.logits.clone()
    # an eager rollout on that store now launches what the replay does -- the new kernels, none of the products they replace
    fresh = follower.FollowerEngine(enc, dec, store)
    with torch.no_grad():
        fresh.rollout(batch, S, 'argmax', train=False)
        torch.cuda.synchronize()
        with _lib.kernel_profile() as prof:
            ref = fresh.rollout(batch, S, 'argmax', train=False)
            torch.cuda.synchronize()
    names = set(prof.rows)
    assert ref.projected
    assert any('pair_proj_textfold_kernel' in k for k in names) and any('pair_proj_score_kernel' in k for k in names)
    assert not [k for k in names if 'pair_apro_small' in k or 'pair_vis_small' in k or 'pair_score_merge' in k]
    assert sum(v['calls'] for k, v in prof.rows.items() if 'pair_proj_' in k) == 2 * S      # two launches per step ...
    assert prof.rows['visual_attn_split_proj_kernel']['calls'] == 1                          # ... and step 0's head is one
    assert not [k for k in names if k.startswith('visual_attn_split_kernel')]
    assert torch.equal(a, ref.logits) and torch.equal(gst.actions, ref.actions)
    # an in-place change of a weight the tables depend on: refreshed in place ahead of the replay
    ptrs = [b.data_ptr() for b in store.projected(dec, build=False)['bufs']]
    with torch.no_grad():
        dec.decoder2action.linear_in_a.weight.mul_(1.25)
        dec.visual_attention_layer.linear_in_v.weight.mul_(0.75)
    replay()
    torch.cuda.synchronize()
    hit = store.projected(dec, build=False)
    assert hit['builds'] == 2 and [b.data_ptr() for b in hit['bufs']] == ptrs
    ref2 = _run(follower.FollowerEngine(enc, dec, store), batch, S)
    assert ref2.projected
    assert torch.equal(gst.logits, ref2.logits) and not torch.equal(gst.logits, a)
    # ... and the four-launch chain agrees with the refreshed tables
    off = follower.FollowerEngine(enc, dec, store)
    off.project = False
    ref3 = _run(off, batch, S)
    assert not ref3.projected and torch.equal(ref3.actions, ref2.actions)
    # a re-allocated weight cannot be patched into the graph
    w = dec.decoder2action.linear_in_a.weight
    w.data = w.data.clone()
    with pytest.raises(follower.WeightsMoved):
        replay()


def test_project_true_builds_on_first_use_and_false_never_uses():
    from speaker_follower_amd import follower
    enc, dec, store, batch = _world(B=17)
    on = follower.FollowerEngine(enc, dec, store)
    on.project = True
    s_on = _run(on, batch, 3)
    assert s_on.projected and store.projected(dec, build=False) is not None
    off = follower.FollowerEngine(enc, dec, store)
    off.project = False
    s_off = _run(off, batch, 3)
    assert not s_off.projected and torch.equal(s_on.actions, s_off.actions)
    replay, gst = off.capture(batch, 3, 'argmax')
    replay()
    torch.cuda.synchronize()
    assert not gst.projected and torch.equal(gst.logits, s_off.logits)


@pytest.mark.parametrize('case', ['B257', 'fp16', 'train', 'differentiable'])
def test_declining_cases_run_the_chain_they_ran_before(case):
    """Never an error, never a half-issued step: identical actions with `project = True` and `project = False`."""
    from speaker_follower_amd import features, follower
    enc, dec, _, _ = _models()
    B = 257 if case == 'B257' else 16
    S = 2
    fb = _edge_batch(B, S)
    store = features.FeatureStore(synth.feature_table(5, NVP), dtype='fp16' if case == 'fp16' else 'fp32')
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    out = {}
    for mode in (True, False):
        eng = follower.FollowerEngine(enc, dec, store)
        eng.project = mode
        if case == 'train':
            st = eng.rollout(batch, S, 'teacher', train=True)
        elif case == 'differentiable':
            st = eng.rollout(batch, S, 'teacher', train=False)
            assert st.differentiable
        else:
            st = _run(eng, batch, S)
        torch.cuda.synchronize()
        assert not st.projected
        out[mode] = (st.actions.cpu().numpy().copy(), st.logits.detach().cpu().numpy().copy())
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
    assert store.projected(dec, build=False) is None              # (nothing was built for a rollout that cannot use it)


def test_device_environment_declines():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import search_world as W
    from speaker_follower_amd import features, follower, nav
    env, table = W.build_world(dense=False, n_items=24, batch=12, item_seed=77)
    enc, dec, _, _ = _models(303)
    store = features.FeatureStore(table)
    nt = nav.NavTable(env, store)
    env.reset_epoch()
    env._next_minibatch(True)
    items = list(env.batch)
    out = {}
    for mode in (True, False):
        eng = follower.FollowerEngine(enc, dec, store)
        eng.project = mode
        st = _run(eng, nav.DeviceNavBatch(nt, items, 5), 5)
        assert st.text_folded and not st.projected
        out[mode] = (st.actions.cpu().numpy().copy(), st.logits.cpu().numpy().copy())
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
