"""GPU: opt-in bf16 weight storage for the decoder's LSTM gate product (include/sf_hip.h: sf_gate_product_bf16_weights;
csrc/sf_gemm.hip: gemm_nt_bf16w_kernel, pack_bf16_kernel; FollowerEngine.gate_weights / Seq2SeqAgent.gate_weights).

The mode changes results (about 1 % of the logit scale on peaky weights), so its correctness is always checked against
arithmetic on the SAME ROUNDED weights -- float64 for the product, the numpy oracle for the rollout -- never against
the fp32-weights path; the fp32-weights path itself must not move by a bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import search_world as W                                               # noqa: E402
from tests.tol import assert_logits_close                              # noqa: E402
from speaker_follower_amd import synth                                 # noqa: E402
from oracle import np_env, np_model                                    # noqa: E402  (checker only)

NEW_KERNEL, OLD_KERNEL = 'gemm_nt_bf16w_kernel', 'gemm_nt_split_kernel'
SCORE_TOL = 3e-4                  # tests/test_gpu_follower_route_scoring.py: the route-scoring tolerance


def bf16_round(t):
    """round-to-nearest-even to bf16 and back, by torch on the CPU (the reference of the pack kernel)."""
    return t.detach().cpu().to(torch.bfloat16).to(torch.float32)


def slabs_product(x, w, h, u, M, N, K1, K2):
    """sf_linear_slabs_fwd -> (the K-split slabs [ks, M, N] (a copy), the names of the kernels it launched)."""
    from speaker_follower_amd._lib import call, kernel_profile
    from speaker_follower_amd.runtime import ptr, ws_args, workspace
    ks = C.c_int(0)
    with kernel_profile() as prof:
        call('sf_linear_slabs_fwd', ptr(x), K1, ptr(w), K1, ptr(h), K2, ptr(u), K2, M, N, C.byref(ks), *ws_args(x.device))
    torch.cuda.synchronize()
    slabs = workspace(x.device)[:ks.value * M * N * 4].view(torch.float32).view(ks.value, M, N).clone()
    return slabs, ' '.join(prof.rows)


# ---------------------------------------------------------------------------------------------------- 1. rounding, layout
def special_bits():
    """fp32 patterns whose rounding to bf16 is the interesting part: exact ties between two bf16 neighbours with the kept
    bit even and odd, their nearest neighbours on both sides, the same far down (2^-120) and in the subnormal range (ties
    there too; the largest subnormal rounds up to the smallest normal), +-0, the largest finite bf16 -- all with both signs."""
    pos = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x40490FDB,
           0x03808000, 0x03818000, 0x03807FFF, 0x03818001,
           0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007F8000, 0x007FFFFF, 0x00800000,
           0x00000000, 0x7F7F0000, 0x7F7E8000, 0x7F7E7FFF]
    return np.array(pos + [b | 0x80000000 for b in pos], np.uint32)


def weights_with_specials(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.05
    sp = torch.from_numpy(special_bits().view(np.int32).copy()).view(torch.float32)
    flat = w.view(-1)
    # scattered with a stride coprime to K: every special value lands in many columns, K halves, lane groups and rows
    pos = (torch.arange(8 * sp.numel()) * 37 + 5) % flat.numel()
    flat[pos] = sp.repeat(8)
    return w


def one_hot_columns(w, u, M, N, K1, K2, starts1, starts2):
    """Rows r of the activation select k = k0 + r of one segment: the summed slabs ARE columns k0 .. k0 + M - 1 of the
    rounded weights.  A sum that starts at +0 cannot end at -0, so a rounded weight of -0 reads back as 0 -- compared by
    value; every other value by value means bit for bit."""
    from speaker_follower_amd import runtime
    from speaker_follower_amd._lib import lib
    dev = torch.device('cuda', 0)
    wd, ud = w.to(dev), u.to(dev)
    want = (bf16_round(w), bf16_round(u))
    runtime.register_bf16_weights(wd, ud)
    assert lib.sf_gate_product_bf16_supported(M, K1, K2, N) == 1
    checked = 0
    with runtime.bf16_gate_weights():
        for seg, starts in ((0, starts1), (1, starts2)):
            K = (K1, K2)[seg]
            for k0 in starts:
                act = [torch.zeros(M, K1, device=dev), torch.zeros(M, K2, device=dev)]
                n = min(M, K - k0)
                act[seg][torch.arange(n), k0 + torch.arange(n)] = 1.0
                slabs, names = slabs_product(act[0], wd, act[1], ud, M, N, K1, K2)
                assert NEW_KERNEL in names and OLD_KERNEL not in names, names
                got = slabs.sum(0).cpu()
                ref = want[seg][:, k0:k0 + n].T.contiguous()
                bad = got[:n] != ref
                assert not bad.any(), ('segment %d, k0 %d: %d of %d differ, first at %s' %
                                       (seg, k0, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist()))
                assert not got[n:].any()                               # the all-zero rows behind the one-hot ones
                nz = ref != 0
                assert torch.equal(got[:n][nz].view(torch.int32), ref[nz].view(torch.int32))
                checked += n
    return checked


@pytest.mark.parametrize('M', [128, 64])
def test_rounding_and_packed_layout_are_exact_for_every_k(M):
    """K1 = 128, K2 = 64, N = 80 (five n-tiles: a partial 64-column block): every k of both segments."""
    N, K1, K2 = 80, 128, 64
    w, u = weights_with_specials(N, K1, 1), weights_with_specials(N, K2, 2)
    sp = set(special_bits().tolist())
    assert sp <= set(w.view(torch.int32).numpy().view(np.uint32).ravel().tolist())      # the special values are in there
    n = one_hot_columns(w, u, M, N, K1, K2, range(0, K1, M), range(0, K2, M))
    assert n == K1 + K2


def test_rounding_and_packed_layout_at_the_real_depth():
    """The same at K1 = 4352, K2 = 512, N = 2048 over a strided sample of k0 (first and last stages, both K splits' seams)."""
    N, K1, K2, M = 2048, 4352, 512, 128
    w, u = weights_with_specials(N, K1, 3), weights_with_specials(N, K2, 4)
    one_hot_columns(w, u, M, N, K1, K2, (0, 1088 + 32, 2176 - 64, 3200 + 8, K1 - M), (0, K2 - M))


def test_pack_kernel_equals_torch_rounding_bit_for_bit():
    """sf_pack_bf16 against torch.Tensor.to(torch.bfloat16): the packed image, un-permuted on the host (the layout is the
    library's own: this test is the one place outside it that spells it out), with a leading dimension wider than K and
    a row count that is no multiple of 16 (the padding rows are zeros)."""
    from speaker_follower_amd._lib import call, lib
    from speaker_follower_amd.runtime import ptr, stream
    R, K, ld = 40, 192, 200
    full = weights_with_specials(R, ld, 5)
    full[1, 1], full[2, 2] = float('inf'), float('-inf')              # (a NaN stays a NaN; torch's own payload differs by backend)
    n = int(lib.sf_pack_bf16_bytes(R, K))
    assert n == 48 * K * 2
    src = full.cuda()
    out = torch.full((n,), 0xAA, dtype=torch.uint8, device='cuda')
    call('sf_pack_bf16', ptr(src), ld, R, K, C.c_void_p(out.data_ptr()), stream())
    torch.cuda.synchronize()
    img = out.cpu().view(torch.int16).view(3, K // 64, 2, 4, 16, 2, 4)          # tile, stage, half, kk, li, e, c
    rows = img.permute(0, 4, 1, 2, 5, 3, 6).reshape(48, K)                     # k = 64 stage + 32 half + 16 e + 4 kk + c
    want = full[:, :K].to(torch.bfloat16).view(torch.int16)
    assert torch.equal(rows[:R], want)
    assert not rows[R:].any()


# ---------------------------------------------------------------------------------------------------- 2. product accuracy
@pytest.fixture(scope='module')
def gate_weights():
    """[W_ih | W_hh] of the decoder LSTM's shape (N = 2048, K = 4352 + 512), registered; their rounded copies."""
    from speaker_follower_amd import runtime
    g = torch.Generator().manual_seed(4864)
    N, K1, K2 = 2048, 4352, 512
    w, u = (torch.randn(N, K1, generator=g) * 0.03), (torch.randn(N, K2, generator=g) * 0.05)
    wd, ud = w.cuda(), u.cuda()
    runtime.register_bf16_weights(wd, ud)
    return dict(N=N, K1=K1, K2=K2, w=wd, u=ud, wr=bf16_round(w).cuda(), ur=bf16_round(u).cuda())


def gate_inputs(M, K1, K2):
    """tests/test_gpu_ops.py: test_gate_product_on_the_bf16_matrix_cores_keeps_fp32_accuracy -- [u | feature] post-ReLU
    non-negative with dropout (x2 or 0), h in (-1, 1): the decoder's LSTM input."""
    g = torch.Generator().manual_seed(M)
    x = (torch.relu(torch.randn(M, K1, generator=g) * 0.5 + 0.4) * 2 * (torch.rand(M, K1, generator=g) < 0.5)).cuda()
    h = torch.tanh(torch.randn(M, K2, generator=g)).cuda()
    return x, h


@pytest.mark.parametrize('M', [1, 16, 17, 100, 128])
def test_product_keeps_fp32_accuracy_on_the_rounded_weights(gate_weights, M):
    """Against float64 on the rounded weights: error <= 2.5e-7 sum |a| |b| -- the bound of the fp32-weights kernel's test
    (the activation side is the same error-free split; bf16 x bf16 products are exact in fp32).  The profile names the
    new kernel with the switch on, the old one with the switch off or without a registration, the fp32 MFMA kernel under
    the strict switch; off, unregistered and strict results are the bits they are without the mode."""
    from speaker_follower_amd import runtime
    from speaker_follower_amd._lib import lib
    gw = gate_weights
    N, K1, K2, w, u = gw['N'], gw['K1'], gw['K2'], gw['w'], gw['u']
    x, h = gate_inputs(M, K1, K2)
    assert lib.sf_gate_product_bf16_supported(M, K1, K2, N) == 1
    ref = x.double() @ gw['wr'].double().T + h.double() @ gw['ur'].double().T
    mag = x.double().abs() @ gw['wr'].double().abs().T + h.double().abs() @ gw['ur'].double().abs().T

    off, names = slabs_product(x, w, h, u, M, N, K1, K2)
    assert OLD_KERNEL in names and NEW_KERNEL not in names, names
    with runtime.bf16_gate_weights():
        on, names = slabs_product(x, w, h, u, M, N, K1, K2)
        assert NEW_KERNEL in names and OLD_KERNEL not in names, names
        w2, u2 = w.clone(), u.clone()                                  # the same values at unregistered addresses
        unreg, names = slabs_product(x, w2, h, u2, M, N, K1, K2)
        assert OLD_KERNEL in names and NEW_KERNEL not in names, names
        with runtime.strict_gate_product():
            strict_on, names = slabs_product(x, w, h, u, M, N, K1, K2)
            assert OLD_KERNEL not in names and NEW_KERNEL not in names, names          # the strict switch wins
    with runtime.strict_gate_product():
        strict_off, _ = slabs_product(x, w, h, u, M, N, K1, K2)
    again, _ = slabs_product(x, w, h, u, M, N, K1, K2)
    assert torch.equal(off, unreg) and torch.equal(off, again) and torch.equal(strict_on, strict_off)
    assert on.shape == off.shape                                       # same K splits: the consumer interface is unchanged

    err = on.sum(0).double() - ref
    rel = float((err.abs() / mag).max())
    err32 = off.sum(0).double() - (x.double() @ w.double().T + h.double() @ u.double().T)
    print('[gate product, bf16 weights, M=%d] vs float64 on the rounded weights: max %.2e  rel %.2e  rms %.2e | fp32-weights '
          'kernel vs float64 on its own weights: max %.2e rms %.2e | bf16 vs fp32 weights: max |d| %.2e'
          % (M, float(err.abs().max()), rel, float(err.pow(2).mean().sqrt()), float(err32.abs().max()),
             float(err32.pow(2).mean().sqrt()), float((on.sum(0) - off.sum(0)).abs().max())))
    assert rel <= 2.5e-7


# ---------------------------------------------------------------------------------------------------- 3. unsupported shapes
def test_unsupported_shapes_run_the_kernels_they_run_without_the_mode(gate_weights):
    from speaker_follower_amd import runtime
    from speaker_follower_amd._lib import lib
    gw = gate_weights
    N, K1, K2 = gw['N'], gw['K1'], gw['K2']
    # more rows than one block holds: the pair is registered, the shape is not supported
    M = 129
    assert lib.sf_gate_product_bf16_supported(M, K1, K2, N) == 0
    x, h = gate_inputs(M, K1, K2)
    off, names_off = slabs_product(x, gw['w'], h, gw['u'], M, N, K1, K2)
    with runtime.bf16_gate_weights():
        on, names_on = slabs_product(x, gw['w'], h, gw['u'], M, N, K1, K2)
    assert names_on == names_off and NEW_KERNEL not in names_on
    assert torch.equal(on, off)
    # a depth that is no multiple of 64: nothing to pack, nothing to register, the call is today's
    M, N2, K1b, K2b = 100, 256, 4352 + 4, 512
    assert lib.sf_gate_product_bf16_supported(M, K1b, K2b, N2) == 0 and lib.sf_pack_bf16_bytes(N2, K1b) == 0
    g = torch.Generator().manual_seed(7)
    w, u = (torch.randn(N2, K1b, generator=g) * 0.03).cuda(), (torch.randn(N2, K2b, generator=g) * 0.05).cuda()
    with pytest.raises(ValueError):
        runtime.register_bf16_weights(w, u)
    x, h = gate_inputs(M, K1b, K2b)
    off, names_off = slabs_product(x, w, h, u, M, N2, K1b, K2b)
    with runtime.bf16_gate_weights():
        on, names_on = slabs_product(x, w, h, u, M, N2, K1b, K2b)
    assert names_on == names_off and NEW_KERNEL not in names_on
    assert torch.equal(on, off)


# ---------------------------------------------------------------------------------------------------- rollouts
def build_follower(enc_w, dec_w):
    from speaker_follower_amd import model
    d = synth.FULL
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    return enc.cuda(), dec.cuda()


@pytest.fixture(scope='module')
def g8(golden):
    """The G8 seeds (tests/test_gpu_hard_parity.py) and the peaky weights they name, built once."""
    g = golden('g8_follower_peaky_b100_argmax')
    seeds = dict(weight=int(g['weight_seed']), batch=int(g['batch_seed']), table=int(g['table_seed']))
    enc_w, dec_w = synth.follower_weights_peaky(seeds['weight'])
    dec_r = dict(dec_w)                                                # what the oracle runs on: the rounded LSTM weights
    for k in ('lstm.weight_ih', 'lstm.weight_hh'):
        dec_r[k] = bf16_round(torch.tensor(dec_w[k])).numpy()
    return seeds, enc_w, dec_w, dec_r


@pytest.mark.parametrize('feedback', ['teacher', 'argmax'])
@pytest.mark.parametrize('shape', [(17, 6, 48), (100, 20, 256)], ids=['b17x6', 'b100x20'])
def test_rollout_equals_the_oracle_on_the_rounded_weights(g8, shape, feedback):
    """np_model.follower_rollout on bf16_rne(lstm.weight_ih / weight_hh): identical actions, logits / h / c / loss within
    what tests/test_gpu_hard_parity.py asks of G8 (1e-4 absolute on the logits, rtol = atol = 1e-4 on h and c, 1e-4
    relative on the loss).  The oracle's smallest top-2 logit gap on these inputs: 1.3e-2 / 2.8e-3 (teacher / argmax) at
    B = 17 x 6, 4.3e-4 / 8.4e-4 at B = 100 x 20 -- of the order of the fp32 G8 test's own.  Prints (no assertion) how far
    the GPU's bf16-weights logits are from its fp32-weights ones."""
    from speaker_follower_amd import features, follower as fol
    seeds, enc_w, dec_w, dec_r = g8
    B, S, NVP = shape
    enc, dec = build_follower(enc_w, dec_w)
    enc.eval()
    dec.eval()
    fb = synth.follower_batch(seed=seeds['batch'], batch=B, steps=S, n_viewpoints=NVP)
    table = synth.feature_table(seeds['table'], NVP)
    eng = fol.FollowerEngine(enc, dec, features.FeatureStore(table))
    batch = fol.DeviceFollowerBatch.from_synth(fb)
    with torch.no_grad():
        st32 = eng.rollout(batch, S, feedback, train=False)
        eng.gate_weights = 'bf16'
        st = eng.rollout(batch, S, feedback, train=False)
    seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, 80, reverse=True)
    loc = np_env.static_loc_embeddings()
    ref = np_model.follower_rollout(enc_w, dec_r, seq, lens, mask, S,
                                    lambda t: np_env.dense_follower_step(table, loc, fb, t),
                                    fb.target, feedback, synth.FULL.feat, early_exit=False)
    lg, lg32 = st.logits.cpu().numpy(), st32.logits.cpu().numpy()
    fin = np.isfinite(lg32)
    top2 = [np.sort(l[np.isfinite(l).sum(1) > 1], axis=1)[:, -2:] for l in ref['logits']]
    gap = min(float((t[:, 1] - t[:, 0]).min()) for t in top2 if len(t))
    print('[bf16 gate weights, B=%d x %d, %s] GPU bf16-weights vs GPU fp32-weights: max|dlogit| = %.3e at max|logit| = %.3f, '
          '%d of %d actions differ; oracle top-2 gap >= %.2e'
          % (B, S, feedback, float(np.abs(lg[fin] - lg32[fin]).max()), float(np.abs(lg32[fin]).max()),
             int((st.actions != st32.actions).sum()), st.actions.numel(), gap))
    assert np.array_equal(st.actions.cpu().numpy(), ref['actions'])
    worst = 0.0
    for t in range(S):
        a = ref['logits'][t].shape[1]
        worst = max(worst, assert_logits_close(lg[t][:, :a], ref['logits'][t],
                                               'bf16-weights rollout B=%d %s, step %d' % (B, feedback, t)))
    np.testing.assert_allclose(st.h.cpu().numpy(), ref['h'], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(st.c.cpu().numpy(), ref['c'], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(float(st.loss), float(ref['loss']), rtol=1e-4)
    assert not torch.equal(st.logits, st32.logits)                     # the mode did something


def small_case(seed=11, B=8, S=10, NVP=48):
    enc_w, dec_w = synth.follower_weights_peaky(seed)
    fb = synth.follower_batch(seed=3, batch=B, steps=S, n_viewpoints=NVP, min_len=6, max_len=30)
    table = synth.feature_table(2, NVP)
    return enc_w, dec_w, fb, table, S


def test_training_ignores_the_mode(g8):
    """gate_weights = 'bf16' on the engine, one training iteration at B = 8 x 10 steps: loss and every gradient are the
    bits of 'fp32', and no launch of the training pass is the new kernel -- although the pair is registered (an inference
    rollout of the same engine has just used it) and although the caller's own switch is on around the pass."""
    from speaker_follower_amd import features, follower as fol, runtime
    from speaker_follower_amd._lib import kernel_profile
    enc_w, dec_w, fb, table, S = small_case()
    out = {}
    for mode in ('fp32', 'bf16'):
        enc, dec = build_follower(enc_w, dec_w)
        eng = fol.FollowerEngine(enc, dec, features.FeatureStore(table))
        eng.dropout_seed = 4242
        eng.gate_weights = mode
        batch = fol.DeviceFollowerBatch.from_synth(fb)
        enc.eval()
        dec.eval()
        with torch.no_grad(), kernel_profile() as prof:
            eng.rollout(batch, S, 'argmax', train=False)
        assert (NEW_KERNEL in ' '.join(prof.rows)) == (mode == 'bf16')
        eng.site_next, eng.iteration = 0, 0                            # (the same dropout sites in both runs)
        enc.train()
        dec.train()
        with runtime.bf16_gate_weights(mode == 'bf16'), kernel_profile() as prof:
            st = eng.rollout(batch, S, 'teacher', train=True)
            st.loss.backward()
            torch.cuda.synchronize()
        names = ' '.join(prof.rows)
        assert NEW_KERNEL not in names and OLD_KERNEL in names, names
        out[mode] = (st.loss.detach().clone(), st.logits.detach().clone(),
                     {k: p.grad.clone() for m in (enc, dec) for k, p in m.named_parameters() if p.grad is not None})
    assert torch.equal(out['fp32'][0], out['bf16'][0]) and torch.equal(out['fp32'][1], out['bf16'][1])
    assert out['fp32'][2].keys() == out['bf16'][2].keys() and len(out['fp32'][2]) >= 16
    for k, gr in out['fp32'][2].items():
        assert torch.equal(gr, out['bf16'][2][k]), k
    assert float(out['fp32'][2]['lstm.weight_ih'].abs().max()) > 0     # (a real backward)


def inference(eng, batch, S):
    with torch.no_grad():
        st = eng.rollout(batch, S, 'argmax', train=False)
    return st.logits.clone(), st.actions.clone(), st.h.clone()


def test_weights_that_change_are_repacked_eagerly_and_under_a_captured_graph():
    """lstm.weight_ih.add_() (what an optimizer step does), then inference again: the bits of a freshly built engine on
    the new weights, and not the bits from before the update -- eagerly and through a captured rollout replayed after the
    update (the packed image is rebuilt in place, ahead of the replay)."""
    from speaker_follower_amd import features, follower as fol
    enc_w, dec_w, fb, table, S = small_case()
    enc, dec = build_follower(enc_w, dec_w)
    enc.eval()
    dec.eval()
    store = features.FeatureStore(table)
    batch = fol.DeviceFollowerBatch.from_synth(fb)
    eng = fol.FollowerEngine(enc, dec, store)
    eng.gate_weights = 'bf16'
    before = inference(eng, batch, S)
    replay, gst = eng.capture(batch, S, 'argmax')
    replay()
    torch.cuda.synchronize()
    assert torch.equal(gst.logits, before[0]) and torch.equal(gst.actions, before[1])
    g = torch.Generator().manual_seed(1)
    delta = (torch.randn(dec.lstm.weight_ih.shape, generator=g) * 0.02).cuda()
    with torch.no_grad():
        dec.lstm.weight_ih.add_(delta)
    after = inference(eng, batch, S)
    replay()
    torch.cuda.synchronize()
    after_graph = (gst.logits.clone(), gst.actions.clone(), gst.h.clone())
    # a freshly built engine over freshly allocated modules that hold the new weights
    enc2, dec2 = build_follower(enc_w, {k: v.detach().cpu().numpy() for k, v in dec.state_dict().items()})
    enc2.eval()
    dec2.eval()
    assert dec2.lstm.weight_ih.data_ptr() != dec.lstm.weight_ih.data_ptr()
    eng2 = fol.FollowerEngine(enc2, dec2, store)
    eng2.gate_weights = 'bf16'
    fresh = inference(eng2, batch, S)
    for a, b, c in zip(after, after_graph, fresh):
        assert torch.equal(a, c) and torch.equal(b, c)
    assert not torch.equal(after[0], before[0])


def test_captured_rollouts_keep_the_mode_they_were_captured_with():
    from speaker_follower_amd import features, follower as fol
    enc_w, dec_w, fb, table, S = small_case()
    enc, dec = build_follower(enc_w, dec_w)
    enc.eval()
    dec.eval()
    batch = fol.DeviceFollowerBatch.from_synth(fb)
    eng = fol.FollowerEngine(enc, dec, features.FeatureStore(table))
    eager32 = inference(eng, batch, S)
    replay32, st32 = eng.capture(batch, S, 'argmax')                    # captured in fp32 mode ...
    eng.gate_weights = 'bf16'                                           # ... and the attribute flipped afterwards
    eager16 = inference(eng, batch, S)
    assert not torch.equal(eager16[0], eager32[0])
    replay16, st16 = eng.capture(batch, S, 'argmax')
    replay16()
    replay32()
    torch.cuda.synchronize()
    assert torch.equal(st16.logits, eager16[0]) and torch.equal(st16.actions, eager16[1]) and torch.equal(st16.h, eager16[2])
    assert torch.equal(st32.logits, eager32[0]) and torch.equal(st32.actions, eager32[1]) and torch.equal(st32.h, eager32[2])
    eng.gate_weights = 'fp32'
    replay16()                                                          # and the other way round
    torch.cuda.synchronize()
    assert torch.equal(st16.logits, eager16[0])
    assert torch.equal(inference(eng, batch, S)[0], eager32[0])


# ---------------------------------------------------------------------------------------------------- search
@pytest.fixture(scope='module')
def world():
    from speaker_follower_amd import agents, features
    env, table = W.build_world(dense=True)
    enc_w, dec_w = synth.follower_weights(W.FOLLOWER_SEED)
    enc, dec = build_follower(enc_w, dec_w)
    agent = agents.Seq2SeqAgent(env, '/tmp/sf_gate_bf16_search.json', enc.eval(), dec.eval(), episode_len=W.EPISODE_LEN)
    agent.store = features.FeatureStore(table)
    return env, agent


def test_step_caches_hold_one_object_per_mode(world):
    from speaker_follower_amd import nav, search
    env, agent = world
    table = nav.table_for(env, agent.store)
    got = {}
    for mode in ('fp32', 'bf16', 'fp32'):
        agent.gate_weights = mode
        gs = search.graph_step_for(agent, table, W.BATCH, 16)
        db = search.follower_beam_for(agent, table, W.BATCH, 3, 2, True)
        assert gs.gate_weights == db.gate_weights == mode
        assert search.graph_step_for(agent, table, W.BATCH, 16) is gs              # (a hit while the mode stays)
        assert search.follower_beam_for(agent, table, W.BATCH, 3, 2, True) is db
        got.setdefault(mode, []).append((gs, db))
    assert got['fp32'][0][0] is not got['bf16'][0][0] and got['fp32'][0][1] is not got['bf16'][0][1]
    assert got['fp32'][1][1] is got['fp32'][0][1]                      # the beam cache keeps both modes side by side
    agent.gate_weights = 'fp32'


def rescored(agent, cands):
    flat = [c for lst in cands for c in lst]
    agent.score_on_device = True
    try:
        with torch.no_grad():
            out, _ = agent._score_obs_actions_and_instructions([c['observations'] for c in flat], [c['actions'] for c in flat],
                                                               [c['instr_encoding'] for c in flat])
    finally:
        agent.score_on_device = False
    return flat, out


def check_against_rescoring(agent, cands, what):
    flat, out = rescored(agent, cands)
    assert len(flat) == len(out) > 0
    worst = 0.0
    for c, r in zip(flat, out):
        assert c['instr_id'] == r['instr_id'] and [int(a) for a in c['actions']] == r['actions']
        assert len(c['scores']) == len(c['actions']) == len(r['scores'])
        np.testing.assert_allclose(c['scores'], r['scores'], rtol=0, atol=1e-4)
        worst = max(worst, abs(c['score'] - r['score']) / max(1.0, abs(r['score'])))
    print('[bf16 gate weights] %s: %d routes, worst relative score difference to the teacher-forced re-scoring %.2e'
          % (what, len(flat), worst))
    assert worst <= SCORE_TOL


def test_searches_run_in_the_mode_and_agree_with_its_route_scoring(world):
    """One beam search (beam 3) and one state-factored search on the small fixture world in bf16 mode: well-formed results,
    the new kernel in the profile of the host-issued steps, and scores that a teacher-forced bf16-mode re-scoring of the
    returned routes reproduces within the route-scoring tolerance."""
    from speaker_follower_amd._lib import kernel_profile
    env, agent = world
    agent.gate_weights = 'bf16'
    try:
        env.set_beam_size(3)
        env.reset_epoch()
        with torch.no_grad(), kernel_profile() as prof:
            trajs, completed, traversed = agent.beam_search(3)
        assert NEW_KERNEL in ' '.join(prof.rows)
        assert len(trajs) == W.BATCH and traversed is None
        for lst in trajs:
            assert 1 <= len(lst) <= 3
            for c in lst:
                assert len(c['trajectory']) >= 1 and len(c['attentions']) == len(c['actions']) <= W.EPISODE_LEN
                assert np.isfinite(c['score']) and c['score'] <= 0
        check_against_rescoring(agent, trajs, 'beam search (3)')

        env.reset_epoch()
        agent.search_graph = False                                     # host-issued steps: visible to the profile
        try:
            with torch.no_grad(), kernel_profile() as prof:
                eager, _, _ = agent.state_factored_search(3, 1)
        finally:
            del agent.search_graph
        assert NEW_KERNEL in ' '.join(prof.rows)
        env.reset_epoch()
        with torch.no_grad():
            trajs, completed, traversed = agent.state_factored_search(3, 1)         # the captured step (GraphStep)
        assert len(trajs) == len(eager) == W.BATCH and len(traversed) == W.BATCH
        for lst, le in zip(trajs, eager):
            assert 1 <= len(lst) <= 3 and [c['actions'] for c in lst] == [c['actions'] for c in le]
            ends = [(c['observations'][-1]['viewpoint'], c['observations'][-1]['heading']) for c in lst]
            assert len(set(ends)) == len(ends)                         # one candidate per end state
        check_against_rescoring(agent, trajs, 'state-factored search (3, 1)')
    finally:
        agent.gate_weights = 'fp32'
