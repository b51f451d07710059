"""GPU: both directions of the bidirectional encoder as ONE persistent launch (csrc/sf_persist.hip: enc_persist_kernel<2>
/ enc_bwd_persist_kernel<2>, through sf_encoder_bilstm_fwd / _bwd) against the per-step kernels of the same entries
(`enc.persistent = False`, SF_ENC_PER_STEP): eval-mode outputs on ragged lengths, the fall-back above the launch's limits,
the G12 golden, a training step's loss, gradients and ctx dropout mask, and the folded text attention of inference
rollouts over a bidirectional context."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402


def _encoder(seed, glove=True):
    from speaker_follower_amd import model
    d = synth.FULL
    w = synth.bidirectional_encoder_weights(seed)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden // 2, 0, 0.5, bidirectional=True,
                            glove=w['embedding.weight'] if glove else None)
    enc.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return enc.cuda()


def _decoder(seed):
    from speaker_follower_amd import model
    d = synth.FULL
    _, dec_w = synth.follower_weights_peaky(seed)
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    return dec.cuda()


def _tokens(B, T, seed):
    """Ragged rows: the first of full length T, the last (B > 1) of one token, the rest anywhere in between."""
    r = np.random.default_rng(seed)
    lens = [int(x) for x in r.integers(1, T + 1, size=B)]
    lens[0] = T
    if B > 1:
        lens[-1] = 1
    seq = np.zeros((B, T), np.int64)
    for b, n in enumerate(lens):
        seq[b, :n] = r.integers(4, synth.FULL.vocab, size=n)
    return torch.tensor(seq).cuda(), lens


def _run(enc, seq, lens, persistent):
    enc.persistent = persistent
    try:
        with torch.no_grad():
            out = enc(seq, lens)
        torch.cuda.synchronize()
        return [o.clone() for o in out], enc.last_path
    finally:
        enc.persistent = True


@pytest.mark.parametrize('B,T', [(1, 80), (37, 80), (100, 80), (128, 80), (1, 128), (37, 128), (100, 128), (128, 128)])
def test_persistent_forward_equals_the_per_step_kernels(B, T):
    enc = _encoder(7).eval()
    seq, lens = _tokens(B, T, seed=B * 1000 + T)
    (ctx_p, h_p, c_p), path_p = _run(enc, seq, lens, True)
    (ctx_s, h_s, c_s), path_s = _run(enc, seq, lens, False)
    assert path_p == 'persistent' and path_s == 'per_step'
    assert ctx_p.shape == (B, T, 512) and h_p.shape == c_p.shape == (B, 512)
    for name, a, b in (('ctx', ctx_p, ctx_s), ('decoder_init', h_p, h_s), ('c_t', c_p, c_s)):
        err = float((a - b).abs().max())
        print('[bidir persistent] B=%d T=%d %s: max abs diff %.2e' % (B, T, name, err))
        assert err <= 2e-6, name
    ctx = ctx_p.cpu().numpy()
    for b, n in enumerate(lens):                                   # pad_packed_sequence: exactly zero beyond the length
        assert not ctx[b, n:].any()
    if B > 1:                                                      # the one-token row: both halves at position 0
        assert np.abs(ctx[-1, 0, :256]).max() > 0 and np.abs(ctx[-1, 0, 256:]).max() > 0


def test_above_the_launch_limits_the_entry_falls_back_to_the_per_step_kernels():
    enc = _encoder(8).eval()
    seq, lens = _tokens(200, 80, seed=200)
    (ctx_p, h_p, c_p), path_p = _run(enc, seq, lens, True)
    (ctx_s, h_s, c_s), path_s = _run(enc, seq, lens, False)
    assert path_p == 'per_step' and path_s == 'per_step'
    assert torch.equal(ctx_p, ctx_s) and torch.equal(h_p, h_s) and torch.equal(c_p, c_s)


def test_golden_g12_through_the_persistent_launch(golden):
    g = golden('g12_encoder_bidir_eval')
    enc = _encoder(int(g['weight_seed'])).eval()
    with torch.no_grad():
        ctx, h, c = enc(torch.tensor(g['seq']).cuda(), [int(x) for x in g['lengths']])
    torch.cuda.synchronize()
    assert enc.last_path == 'persistent'
    for name, got, want in (('ctx', ctx, g['ctx']), ('decoder_init', h, g['decoder_init']), ('c_t', c, g['c_t'])):
        err = np.abs(got.cpu().numpy() - want).max()
        assert err <= 2e-5, '%s: max abs err %.3g' % (name, err)


def test_training_step_persistent_equals_the_per_step_kernels():
    """GloVe encoder, dropout 0.5 on ctx and in the decoder, teacher feedback, one rollout + backward through the engine:
    the loss, every gradient of both directions, of encoder2decoder and of the decoder, and the ctx dropout mask.
    The encoder's gradients agree within 1e-5 of their largest element.  The decoder's are bounded at 2e-5, the bound of
    the unidirectional launch's weight gradients (tests/test_gpu_persistent.py): they sit behind a context that differs
    by fp32 roundoff (the two paths sum the recurrent product in different orders); measured up to 1.08e-5 of their
    scale (the visual attention's linear_in_v weight, the LSTM biases summed over all S x B rows)."""
    from speaker_follower_amd import features, follower as fol
    S, NVP = 6, 96
    fb = synth.follower_batch(seed=17, batch=64, steps=S, n_viewpoints=NVP, min_len=1, max_len=60, stop_prob=0.05)
    store = features.FeatureStore(synth.feature_table(6, NVP))
    batch = fol.DeviceFollowerBatch.from_synth(fb)
    out = {}
    for persistent in (True, False):
        enc, dec = _encoder(11).train(), _decoder(616).train()
        enc.persistent = persistent
        eng = fol.FollowerEngine(enc, dec, store)
        eng.dropout_seed = 4242
        st = eng.rollout(batch, S, 'teacher', train=True)
        st.loss.backward()
        torch.cuda.synchronize()
        assert enc.last_path == enc.last_backward_path == ('persistent' if persistent else 'per_step')
        grads = {'enc/' + k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
        grads.update({'dec/' + k: p.grad.clone() for k, p in dec.named_parameters() if p.grad is not None})
        out[persistent] = (float(st.loss.detach()), grads, st.ctx.clone())
    (lp, gp, cp), (ls, gs, cs) = out[True], out[False]
    np.testing.assert_allclose(lp, ls, rtol=1e-5)
    for k in ('enc/lstm.weight_hh_l0', 'enc/lstm.weight_hh_l0_reverse', 'enc/lstm.weight_ih_l0_reverse',
              'enc/lstm.bias_ih_l0_reverse', 'enc/encoder2decoder.weight', 'dec/lstm.weight_hh'):
        assert k in gp, k
    assert sorted(gp) == sorted(gs)
    top = max(float(g.abs().max()) for g in gs.values())
    for k in gp:
        scale = float(gs[k].abs().max())
        err = float((gp[k] - gs[k]).abs().max())
        if scale < 1e-6 * top:       # (zero up to roundoff: the scoring's linear_in_a bias; the softmax cannot see a shift)
            assert err <= 1e-7 * top, '%s: %.2e' % (k, err)
            continue
        print('[bidir training step] %-36s %.2e of its largest element' % (k, err / scale))
        assert err <= (1e-5 if k.startswith('enc/') else 2e-5) * scale, '%s: %.2e of %.2e' % (k, err, scale)
    # the dropout mask of the assembled ctx: the same zeros (a kept element of a live position is never exactly 0)
    assert torch.equal(cp == 0, cs == 0)
    lens = batch.lengths
    live = torch.zeros_like(cp, dtype=torch.bool)
    for b, n in enumerate(lens):
        live[b, :n] = True
    dropped = float(((cp == 0) & live).sum()) / float(live.sum())
    assert 0.4 < dropped < 0.6, dropped


@pytest.mark.parametrize('B,S,min_len,max_len', [(100, 8, 10, 79), (37, 5, 3, 30), (16, 3, 2, 12)])
def test_folded_text_attention_with_a_bidirectional_context(B, S, min_len, max_len):
    from speaker_follower_amd import features, follower as fol
    enc, dec = _encoder(13).eval(), _decoder(717).eval()
    NVP = 96
    fb = synth.follower_batch(seed=31 + B, batch=B, steps=S, n_viewpoints=NVP, min_len=min_len, max_len=max_len)
    store = features.FeatureStore(synth.feature_table(5, NVP))
    batch = fol.DeviceFollowerBatch.from_synth(fb)
    res = {}
    for fold in (True, False):
        eng = fol.FollowerEngine(enc, dec, store)
        eng.fold_text = fold
        with torch.no_grad():
            st = eng.rollout(batch, S, 'argmax', train=False)
        torch.cuda.synchronize()
        assert bool(getattr(st, 'text_folded', False)) == fold
        assert enc.last_path == 'persistent'
        res[fold] = (st.logits.cpu().numpy().copy(), st.actions.cpu().numpy().copy())
    (lf, af), (lu, au) = res[True], res[False]
    fin = np.isfinite(lu)
    assert np.array_equal(fin, np.isfinite(lf))
    scale = float(np.abs(lu[fin]).max())
    d = float(np.abs(lf[fin] - lu[fin]).max())
    print('[bidir text fold] B=%d S=%d: max |logit| %.2f, folded vs unfolded %.2e' % (B, S, scale, d))
    assert 0 < d <= 3e-5 * max(scale, 1.0)
    assert np.array_equal(af, au)
