"""GPU: fp16 storage of the feature table (features.FeatureStore(dtype='fp16'), include/sf_hip.h: sf_feature_table_f16).

fp16 -> fp32 widening is exact, so the feature has a sharp definition: a store with fp16 storage behaves, BIT FOR BIT, like
the fp32 store built from `table.half().float()`, in every forward and backward entry point.  Every case below builds the
two stores from one array (`_stores`) and compares them with torch.equal -- no tolerance: a difference is an addressing or
conversion bug, not rounding noise.  The one comparison with UNROUNDED features is the G4 case at the end."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402
from oracle import np_env, np_model                                   # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _pool_cycle():
    """torch hands out its pooled stream handles round-robin: [first, ..., last] of one full turn, or None."""
    seen = [torch.cuda.Stream().cuda_stream]
    while len(seen) <= 256:
        h = torch.cuda.Stream().cuda_stream
        if h == seen[0]:
            return seen
        seen.append(h)
    return None


@pytest.fixture(scope='module', autouse=True)
def _leave_the_process_as_this_module_found_it():
    """The captures, searches and two-stream backwards below run on many streams, and runtime.workspace keeps one 64 MB
    scratch buffer per stream HANDLE for the life of the process (torch hands out a few pooled handles, round-robin).
    Every graph and engine made here is gone when the module ends, so the buffers it caused are handed back and the pool
    is turned on to where it stood: the tests that follow get the handles, with or without a workspace, that they get
    when this module is not run."""
    from speaker_follower_amd import runtime
    before, probed = set(runtime._workspaces), set(runtime._concurrent)
    cycle = _pool_cycle()                                  # (one full turn and one: the next handle is cycle[1])
    yield
    gc.collect()
    torch.cuda.synchronize()
    for key in set(runtime._workspaces) - before:
        del runtime._workspaces[key]
    for key in set(runtime._concurrent) - probed:          # (side streams probed here: the next user probes as it would have)
        del runtime._concurrent[key]
    if cycle:
        for _ in range(len(cycle) + 1):
            if torch.cuda.Stream().cuda_stream == cycle[-1]:        # the next one handed out is cycle[0] again
                break


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _rounded(t):
    return torch.from_numpy(np.ascontiguousarray(t, np.float32)).half().float().numpy()


def _stores(t, loc=128):
    from speaker_follower_amd import features
    s16 = features.FeatureStore(t, dtype='fp16', loc=loc)
    s32 = features.FeatureStore(_rounded(t), loc=loc)
    assert s16.table.dtype == torch.float16 and s32.table.dtype == torch.float32 and s16.dtype == 'fp16'
    assert torch.equal(s16.table.float(), s32.table)
    return s16, s32


def _distinct_table(n, V, IMG):
    """fp32 [n, V, IMG], a distinct value at every (row, view, column), whose roundings walk through EVERY finite
    non-negative fp16 number (zero, all subnormals, 65504) with a stride coprime to the row sizes: element k holds fp16
    pattern (k * 7919) mod 31744 plus (k // 31744) / 64 of that pattern's ulp -- exact in fp32, below the rounding tie."""
    k = np.arange(n * V * IMG, dtype=np.int64)
    bits = ((k * 7919) % 31744).astype(np.uint16)
    h = bits.view(np.float16).astype(np.float32)
    ulp = np.exp2(np.maximum(bits >> 10, 1).astype(np.float32) - 25.0)
    lap = (k // 31744).astype(np.float32)
    assert lap.max() < 32
    t = (h + lap * ulp / 64.0).astype(np.float32).reshape(n, V, IMG)
    t[n - 1, V - 1, IMG - 4:] = [65504.0, 2.0 ** -24, 1023 * 2.0 ** -24, 0.0]     # (the table's very last chunk)
    assert len(np.unique(t[:, :, :IMG - 4])) == t[:, :, :IMG - 4].size
    return t


# ---------------------------------------------------------------------------------------------------------- 1. gathers
@pytest.mark.parametrize('IMG,LOC', [(2048, 128), (8, 128)])
def test_gathers_equal_the_fp32_store_and_a_torch_index_expression(IMG, LOC):
    from speaker_follower_amd import features, _lib
    from speaker_follower_amd.runtime import ptr, stream
    n, V, A = 8, 36, 4
    t = _distinct_table(n, V, IMG)
    s16, s32 = _stores(t, LOC)
    Wd = s32.table
    assert float(Wd.max()) == 65504.0 and bool(((Wd > 0) & (Wd < 6e-5)).any())        # the maximum and subnormals are there
    g = LOC // 4
    # the LAST table row with view V - 1 (an fp32-stride address or a read past the end shows here), vp < 0, row 0
    vp = dev(np.array([n - 1, -1, 0, n - 1, 3, 5], np.int32))
    view = dev(np.array([V - 1, 0, 3, 0, 17, 35], np.int32))
    B = vp.shape[0]
    cand_view = dev(np.array([[V - 1, V - 1, 0, V - 1], [1, 2, 3, 4], [0, 5, 6, 7], [9, V - 1, V - 1, V - 1],
                              [0, 35, 34, 33], [2, 0, 1, 2]], np.int32))
    a_num = dev(np.array([4, 3, 1, 2, 4, 3], np.int32))                     # candidates at and past a_num
    rng = np.random.default_rng(3)
    sincos = dev(features.cand_sincos(rng.uniform(-3, 3, (B, A)), rng.uniform(-0.5, 0.5, (B, A))))
    act = dev(np.array([1, 1, 0, -1, 1, 1], np.int32))                       # act <= 0
    act_view = dev(np.array([V - 1, 4, 2, 7, V - 1, 0], np.int32))
    act_sc = sincos[:, 1].contiguous()

    def run(s):
        out = [s.gather_panorama(vp, view), *s.gather_candidates(vp, cand_view, sincos, a_num),
               s.gather_actions(vp, act_view, act_sc, act)]
        pa = torch.full((B, s.F + 4), -7.0, device='cuda')                 # (strided rows: ld_out > F)
        _lib.call('sf_gather_path_actions', ptr(s.table), s.V, s.IMG, s.LOC, ptr(vp), ptr(act_view), ptr(act_sc), ptr(act),
                  B, ptr(pa), s.F + 4, stream())
        torch.cuda.synchronize()
        return out + [pa]

    r16, r32 = run(s16), run(s32)
    for a, b in zip(r16, r32):
        assert torch.equal(a, b)
    # ... and a torch index expression on the widened table
    live = (vp >= 0)
    vpc = vp.clamp(min=0).long()
    pano = torch.cat((Wd[vpc], s32.loc_table[view.long()]), -1)
    pano = torch.where(live[:, None, None], pano, torch.zeros_like(pano))
    assert torch.equal(r16[0], pano)
    ar = torch.arange(A, device='cuda')[None, :]
    ok = live[:, None] & (ar > 0) & (ar < a_num[:, None])
    cands = torch.cat((Wd[vpc[:, None], cand_view.long()], sincos.repeat_interleave(g, -1)), -1)
    cands = torch.where(ok[:, :, None], cands, torch.zeros_like(cands))
    assert torch.equal(r16[1], cands)
    assert torch.equal(r16[2], (ar < a_num[:, None]).float())
    acts = torch.cat((Wd[vpc, act_view.long()], act_sc.repeat_interleave(g, -1)), -1)
    acts = torch.where((live & (act > 0))[:, None], acts, torch.zeros_like(acts))
    assert torch.equal(r16[3], acts)
    assert torch.equal(r16[4][:, :s16.F], acts) and bool((r16[4][:, s16.F:] == -7.0).all())
    assert bool((r16[3][0, :IMG] == Wd[n - 1, V - 1]).all()) and float(r16[3][0, IMG - 4]) == 65504.0


# --------------------------------------------------------------------------------- 2. attention and scoring kernels alone
@pytest.mark.parametrize('B', [1, 3, 37, 100])
def test_attention_and_scoring_kernels_alone(B):
    from speaker_follower_amd import features, ops
    d = synth.FULL
    NVP, V, F, H, D = 16, d.views, d.feat, d.hidden, 256
    s16, s32 = _stores(synth.feature_table(21, NVP))
    rng = np.random.default_rng(100 + B)
    rnd = lambda *s: dev((rng.standard_normal(s) * 0.1).astype(np.float32))          # noqa: E731
    vp_h = rng.integers(0, NVP, B).astype(np.int32)
    vp_h[0] = NVP - 1
    view_h = rng.integers(0, V, B).astype(np.int32)
    view_h[0] = V - 1
    if B > 2:
        vp_h[2] = -1                                                   # (a padded speaker step: all-zero panorama)
    vp, view = dev(vp_h), dev(view_h)
    h, dout = rnd(B, H), rnd(B, F)
    wv = [rnd(D, H), rnd(D), rnd(D, F), rnd(D)]

    def visual(s):
        out, alpha, t_v, q = ops.visual_attention_fwd(wv, s.pano(vp, view), B, V, F, h)
        g = [torch.zeros_like(a) for a in wv]
        dh = ops.visual_attention_bwd(wv, g, s.pano(vp, view), B, h, alpha, t_v, dout)        # visual_attn mode 1
        torch.cuda.synchronize()
        return [out, alpha, t_v, q, dh] + g

    for a, b in zip(visual(s16), visual(s32)):
        assert torch.equal(a, b)

    ws = [rnd(D, H), rnd(D), rnd(D, F), rnd(D), rnd(1, D), rnd(1)]
    for A in (1, 16):
        cv = rng.integers(0, V, (B, A)).astype(np.int32)
        cv[0, :] = V - 1
        an = rng.integers(1, A + 1, B).astype(np.int32)
        an[0] = A
        idx = [vp, dev(cv), dev(features.cand_sincos(rng.uniform(-3, 3, (B, A)), rng.uniform(-0.5, 0.5, (B, A)))), dev(an)]
        dlogit = rnd(B, A)

        def scoring(s):
            logit, t_a, wt, r = ops.eltwise_prod_scoring_fwd(ws, s.cands(*idx, A), B, A, F, h)
            g = [torch.zeros_like(a) for a in ws]
            dh = ops.eltwise_prod_scoring_bwd(ws, g, s.cands(*idx, A), B, h, t_a, wt, dlogit)   # score_bwd
            torch.cuda.synchronize()
            return [logit, t_a, wt, r, dh] + g

        for a, b in zip(scoring(s16), scoring(s32)):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 3. rollouts
def _follower(peaky_seed=77, train=False):
    from speaker_follower_amd import model
    d = synth.FULL
    enc_w, dec_w = synth.follower_weights_peaky(peaky_seed) if peaky_seed else synth.follower_weights(101)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    enc, dec = enc.cuda(), dec.cuda()
    return (enc.train(), dec.train(), enc_w, dec_w) if train else (enc.eval(), dec.eval(), enc_w, dec_w)


CHAINS = [False, True]            # unfolded, folded four-launch (the three-launch chain, the third, is retired)


@pytest.mark.parametrize('feedback', ['argmax', 'teacher'])
@pytest.mark.parametrize('B', [3, 37])
def test_rollouts_on_host_batches_in_all_three_chains(B, feedback):
    from speaker_follower_amd import follower
    S, NVP = 6, 64
    enc, dec, enc_w, dec_w = _follower()
    fb = synth.follower_batch(seed=40 + B, batch=B, steps=S, n_viewpoints=NVP, min_len=3, max_len=30)
    table = synth.feature_table(9, NVP)
    s16, s32 = _stores(table)
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, 80, reverse=True)
    loc = np_env.static_loc_embeddings()
    rt = _rounded(table)
    ref = np_model.follower_rollout(enc_w, dec_w, seq, lens, mask, S, lambda t: np_env.dense_follower_step(rt, loc, fb, t),
                                    fb.target, feedback, 2176, early_exit=False)
    n = len(ref['logits'])
    for fold in CHAINS:
        res = []
        for s in (s16, s32):
            eng = follower.FollowerEngine(enc, dec, s)
            eng.fold_text = fold
            with torch.no_grad():
                st = eng.rollout(batch, S, feedback, train=False)
            torch.cuda.synchronize()
            res.append((st.logits.clone(), st.actions.clone(), st.loss_buf.clone()))
        for a, b in zip(*res):
            assert torch.equal(a, b), fold
        lg, ac = res[0][0].cpu().numpy(), res[0][1].cpu().numpy()
        assert np.array_equal(ac[:n], ref['actions'])                # the oracle on the ROUNDED table: actions identical,
        for t in range(n):                                           # logits within the existing parity bound
            a = ref['logits'][t].shape[1]
            ok = np.isfinite(ref['logits'][t])
            assert float(np.abs(lg[t][:, :a][ok] - ref['logits'][t][ok]).max()) <= 1e-4


@pytest.mark.parametrize('feedback', ['argmax', 'teacher'])
@pytest.mark.parametrize('B', [3, 37])
def test_rollouts_on_a_device_environment_in_all_three_chains(B, feedback):
    import search_world as W
    from speaker_follower_amd import follower, nav
    env, table = W.build_world(dense=False, n_items=B, batch=B, item_seed=70 + B)
    enc, dec, _, _ = _follower(303)
    s16, s32 = _stores(table)
    env.reset_epoch()
    env._next_minibatch(True)
    items = list(env.batch)
    for fold in CHAINS:
        res = []
        for s in (s16, s32):
            nt = nav.NavTable(env, s)
            eng = follower.FollowerEngine(enc, dec, s)
            eng.fold_text = fold
            navb = nav.DeviceNavBatch(nt, items, 6)
            with torch.no_grad():
                st = eng.rollout(navb, 6, feedback, train=False)
            torch.cuda.synchronize()
            res.append((st.logits.clone(), st.actions.clone(), navb.row.clone(), navb.view.clone()))
        for a, b in zip(*res):
            assert torch.equal(a, b), fold


# ------------------------------------------------------------------------------------------------------------ 5. training
def _grads(mods):
    return [p.grad.clone() for m in mods for p in m.parameters() if p.grad is not None]


@pytest.mark.parametrize('feedback', ['teacher', 'sample'])
def test_one_follower_training_iteration_and_its_captured_replay(feedback):
    from speaker_follower_amd import follower as fol, optim
    B, S, NVP = 8, 6, 64
    fb = synth.follower_batch(seed=3, batch=B, steps=S, n_viewpoints=NVP, min_len=8, max_len=40)
    stores = _stores(synth.feature_table(3, NVP))
    batch = fol.DeviceFollowerBatch.from_synth(fb)
    eager, graph = [], []
    for s in stores:
        enc, dec, _, _ = _follower(21, train=True)
        eng = fol.FollowerEngine(enc, dec, s)
        eng.dropout_seed = 777
        st = eng.rollout(batch, S, feedback, train=True)
        st.loss.backward()
        torch.cuda.synchronize()
        g = _grads((enc, dec))
        assert len(g) > 10 and all(bool(torch.isfinite(x).all()) for x in g)
        eager.append([st.loss.detach().clone(), st.actions.clone()] + g)
        # the same iteration as a capture_training replay over two minibatches (iteration 1 runs eagerly, 2 is a replay)
        enc, dec, _, _ = _follower(21, train=True)
        oe = optim.FusedAdam([p for p in enc.parameters() if p.requires_grad], lr=1e-3, weight_decay=5e-4)
        od = optim.FusedAdam([p for p in dec.parameters() if p.requires_grad], lr=1e-3, weight_decay=5e-4)
        eng = fol.FollowerEngine(enc, dec, s)
        eng.dropout_seed = 777
        tg = eng.capture_training(batch, S, feedback, optimizers=(oe, od))
        first = [tg.first.loss_buf.clone(), tg.first.actions.clone()]
        st2 = tg.replay()
        torch.cuda.synchronize()
        graph.append(first + [st2.loss_buf.clone(), st2.actions.clone()] +
                     [p.detach().clone() for m in (enc, dec) for p in m.parameters()])
    for a, b in zip(*eager):
        assert torch.equal(a, b)
    for a, b in zip(*graph):
        assert torch.equal(a, b)


def _speaker(train):
    from speaker_follower_amd import model
    d = synth.FULL
    senc_w, sdec_w = synth.speaker_weights_peaky(404)
    enc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    dec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    enc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    enc, dec = enc.cuda(), dec.cuda()
    return (enc.train(), dec.train()) if train else (enc.eval(), dec.eval())


def test_one_speaker_training_iteration_and_greedy_decoding():
    from speaker_follower_amd import speaker
    B, S = 6, 24
    sb = synth.speaker_batch(seed=5, batch=B, n_viewpoints=64, min_len=5, max_len=S - 1)
    stores = _stores(synth.feature_table(8, 64))
    batch = speaker.DeviceSpeakerBatch.from_synth(sb)
    train, greedy = [], []
    for s in stores:
        enc, dec = _speaker(True)
        eng = speaker.SpeakerEngine(enc, dec, s)
        eng.dropout_seed = 4321
        st = eng.score(batch, S, 'teacher', train=True)
        st.loss.backward()
        torch.cuda.synchronize()
        g = _grads((enc, dec))
        assert len(g) > 6 and all(bool(torch.isfinite(x).all()) for x in g)
        train.append([st.loss.detach().clone()] + g)
        enc, dec = _speaker(False)                               # 6. encoder + greedy decode
        with torch.no_grad():
            st = speaker.SpeakerEngine(enc, dec, s).score(batch, S, 'argmax', train=False)
        torch.cuda.synchronize()
        greedy.append([st.ctx.clone(), st.words.clone(), st.logits.clone()])
    for a, b in zip(*train):
        assert torch.equal(a, b)
    for a, b in zip(*greedy):
        assert torch.equal(a, b)


# -------------------------------------------------------------------------------------------------------------- 6. search
def _flat(trajs):
    return [(c['instr_id'], [int(a) for a in c['actions']], float(c['score']), [float(x) for x in c['scores']],
             [p[0] for p in c['trajectory']]) for tl in trajs for c in tl]


def test_beam_search_and_state_factored_search_give_identical_results():
    import search_world as W
    from speaker_follower_amd import agents
    out = []
    for which in (0, 1):
        env, table = W.build_world(dense=False)
        enc, dec, _, _ = _follower(0)
        agent = agents.Seq2SeqAgent(env, '/tmp/sf_fp16_search.json', enc, dec, episode_len=W.EPISODE_LEN)
        agent.store = _stores(table)[which]
        with torch.no_grad():
            env.set_beam_size(3)
            env.reset_epoch()
            beams, _, _ = agent.beam_search(3)
            env.set_beam_size(4)
            env.reset_epoch()
            sfs, _, trav = agent.state_factored_search(4, 1)
        out.append((_flat(beams), _flat(sfs), [[s.world_state.viewpointId for s in tr] for tr in trav]))
    assert len(out[0][0]) >= W.BATCH and len(out[0][1]) >= W.BATCH
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------------------------------ 7. lifetime
def test_an_fp32_store_after_a_collected_fp16_store_behaves_like_a_fresh_one():
    from speaker_follower_amd import features, follower, _lib
    S, NVP, B = 4, 48, 12
    enc, dec, _, _ = _follower()
    fb = synth.follower_batch(seed=8, batch=B, steps=S, n_viewpoints=NVP, min_len=3, max_len=20)
    table = synth.feature_table(13, NVP)
    batch = follower.DeviceFollowerBatch.from_synth(fb)

    def run(store):
        with torch.no_grad():
            st = follower.FollowerEngine(enc, dec, store).rollout(batch, S, 'argmax', train=False)
        torch.cuda.synchronize()
        return st.logits.clone(), st.actions.clone()

    first = features.FeatureStore(table)
    want = run(first)                                              # before any fp16 store of this size existed
    del first
    gc.collect()
    s16 = features.FeatureStore(table, dtype='fp16')
    addr16 = s16.table.data_ptr()
    assert _lib.lib.sf_feature_table_is_f16(C.c_void_p(addr16)) == 1
    got16 = run(s16)
    del s16
    gc.collect()
    assert _lib.lib.sf_feature_table_is_f16(C.c_void_p(addr16)) == 0       # weakref.finalize forgot it
    # fp32 stores of the same size until the allocator has had every chance to reuse the fp16 table's block
    keep = [features.FeatureStore(table) for _ in range(3)]
    for s in keep:
        assert _lib.lib.sf_feature_table_is_f16(C.c_void_p(s.table.data_ptr())) == 0
        got = run(s)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ref16 = run(features.FeatureStore(_rounded(table)))
    assert torch.equal(got16[0], ref16[0]) and torch.equal(got16[1], ref16[1])


# ------------------------------------------------------------------------- 4. distance from the UNROUNDED features (G4)
def test_distance_from_the_unrounded_features_on_golden_g4_b100(golden):
    """The one case that compares the fp16 store with an UNROUNDED fp32 reference: golden G4, batch 100, 20 steps, argmax.
    |hip16 - golden| <= 1e-4 + max |oracle(rounded table) - oracle(table)|, the second term from the numpy oracle on the
    CPU.  Actions need not be identical (a rounded table is a different input)."""
    from speaker_follower_amd import features, follower
    g = golden('g4_rollout_b100_argmax')
    S = 20
    n = int(g['n_steps'])
    fb = synth.follower_batch(seed=0, batch=100, steps=S, n_viewpoints=256)
    table = synth.feature_table(0, 256)
    enc, dec, enc_w, dec_w = _follower(0)
    with torch.no_grad():
        st = follower.FollowerEngine(enc, dec, features.FeatureStore(table, dtype='fp16')).rollout(
            follower.DeviceFollowerBatch.from_synth(fb), S, 'argmax')
    torch.cuda.synchronize()
    seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, 80, reverse=True)
    loc = np_env.static_loc_embeddings()
    ora = {}
    for name, tb in (('exact', table), ('rounded', _rounded(table))):
        r = np_model.follower_rollout(enc_w, dec_w, seq, lens, mask, S, lambda t: np_env.dense_follower_step(tb, loc, fb, t),
                                      fb.target, 'argmax', 2176, early_exit=False)
        ora[name] = r
    ref = g['logits']
    A = min(ref.shape[2], st.logits.shape[2])
    lg = st.logits.cpu().numpy()[:n, :, :A]
    fin = np.isfinite(ref[:, :, :A]) & np.isfinite(lg)
    d_hip = float(np.abs(lg[fin] - ref[:, :, :A][fin]).max())
    d_ora = 0.0
    for t in range(min(len(ora['exact']['logits']), len(ora['rounded']['logits']))):
        a, b = ora['exact']['logits'][t], ora['rounded']['logits'][t]
        ok = np.isfinite(a) & np.isfinite(b)
        d_ora = max(d_ora, float(np.abs(a[ok] - b[ok]).max()))
    n_act = int((st.actions.cpu().numpy()[:n] != g['actions']).sum())
    print('[fp16 table, G4 b100 argmax] max |hip16 - golden| = %.3e, max |oracle(rounded) - oracle(exact)| = %.3e, '
          'differing actions: %d of %d' % (d_hip, d_ora, n_act, g['actions'].size))
    assert np.array_equal(np.isfinite(ref[:, :, :A]), np.isfinite(lg))
    assert d_hip <= 1e-4 + d_ora
