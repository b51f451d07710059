"""CPU: the float64 oracle that tests/test_gpu_grads_f64.py measures the training gradients against.

* `torch.autograd.gradcheck` in float64 at tiny dims (H 8, feature width 12, 4 views, context 5, 3 candidates, vocab 11,
  3 decode steps / 4 words) of every function that test differentiates: the follower rollout under teacher forcing with
  dropout masks and a row that ends early, `speaker_score` under teacher forcing with train-mode masks (plain and att-feed
  decoder), the bidirectional encoder and the trainable-embedding encoder with its dropout -- the analytic (autograd)
  gradient of every weight element agrees with finite differences, so the float64 reference is trustworthy element by
  element, not only by norm;
* the new restatements pinned in fp32 against the goldens the reference itself produced: G11 (trainable embeddings),
  G12 (bidirectional encoder) and G14 (att-feed speaker decoder).
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import np_env, rng as orng, torch_ref
from speaker_follower_amd import synth

TINY = dataclasses.replace(synth.SMALL, hidden=8, img=8, loc=4, dot=6, word=6, vocab=11, views=4)
B, T, A, S = 4, 5, 3, 3
F64 = torch.float64


def _mask(r, *shape):
    return torch.tensor((r.random(shape) >= 0.5) * 2.0, dtype=F64)


def _gradcheck(fn, weights):
    """gradcheck of the scalar fn(weights) with respect to every weight tensor (float64, every element)."""
    names = [k for k, v in weights.items() if v.requires_grad]

    def f(*ws):
        w = dict(weights)
        w.update(zip(names, ws))
        return fn(w)
    assert torch.autograd.gradcheck(f, tuple(weights[k] for k in names), eps=1e-6, atol=1e-7, rtol=1e-5)


def _follower_inputs(seed):
    r = np.random.default_rng(seed)
    lens = [5, 4, 2, 1]
    seq = np.zeros((B, T), np.int64)
    for b, n in enumerate(lens):
        seq[b, :n] = r.integers(4, TINY.vocab, size=n)
    ctx_mask = torch.tensor(seq == 0)
    X = r.standard_normal((S, B, TINY.views, TINY.feat))
    U = r.standard_normal((S, B, A, TINY.feat))
    valid = np.ones((S, B, A), np.float32)
    valid[:, 3, 2] = 0
    targets = r.integers(1, A - 1, size=(S, B))
    targets[1, 1] = 0                                          # row 1 stops at step 1: no loss, no gradient after it
    targets[:, 2] = np.where(np.arange(S) >= 2, -1, targets[:, 2])
    return seq, lens, ctx_mask, (X, U, valid), torch.tensor(targets)


def _follower_loss(enc, dec, inputs, drop, drop_emb=None):
    seq, lens, ctx_mask, (X, U, valid), targets = inputs
    res = torch_ref.follower_rollout(enc, dec, torch.tensor(seq), lens, ctx_mask, S,
                                     lambda t: (X[t], U[t], valid[t]), targets, 'teacher', TINY.feat,
                                     drop_masks=drop, drop_emb=drop_emb)
    return res['loss']


def test_gradcheck_follower_rollout_teacher_with_dropout_and_an_early_stop():
    enc_w, dec_w = synth.follower_weights(3, TINY)
    enc = torch_ref.to_torch(enc_w, True, frozen=('embedding.weight',), dtype=F64)
    dec = torch_ref.to_torch(dec_w, True, dtype=F64)
    inputs = _follower_inputs(4)
    r = np.random.default_rng(5)
    m = {t: (_mask(r, B, 2 * TINY.feat), _mask(r, B, TINY.hidden)) for t in range(S)}
    m['ctx'] = _mask(r, B, T, TINY.hidden)
    res = torch_ref.follower_rollout(enc, dec, torch.tensor(inputs[0]), inputs[1], inputs[2], S,
                                     lambda t: tuple(a[t] for a in inputs[3]), inputs[4], 'teacher', TINY.feat,
                                     drop_masks=m.__getitem__)
    assert len(res['logits']) == S and res['loss'].dtype == F64 and res['ctx'].dtype == F64
    _gradcheck(lambda w: _follower_loss(enc, w, inputs, m.__getitem__), dec)
    _gradcheck(lambda w: _follower_loss(w, dec, inputs, m.__getitem__), enc)


def test_gradcheck_trainable_embedding_encoder_with_embedding_dropout():
    enc_w, dec_w = synth.follower_weights(6, TINY)
    enc = torch_ref.to_torch(enc_w, True, dtype=F64)
    dec = torch_ref.to_torch(dec_w, dtype=F64)
    inputs = _follower_inputs(7)
    r = np.random.default_rng(8)
    m = {t: (_mask(r, B, 2 * TINY.feat), _mask(r, B, TINY.hidden)) for t in range(S)}
    m['ctx'] = _mask(r, B, T, TINY.hidden)
    d_emb = _mask(r, B, T, TINY.word)
    _gradcheck(lambda w: _follower_loss(w, dec, inputs, m.__getitem__, d_emb), enc)
    loss = _follower_loss(enc, dec, inputs, m.__getitem__, d_emb)
    loss.backward()
    g = enc['embedding.weight'].grad
    used = set(inputs[0][inputs[0] > 0].tolist())
    for tok in range(TINY.vocab):                               # padding and absent tokens: exactly zero
        assert (float(g[tok].abs().max()) > 0) == (tok in used), tok


def test_gradcheck_bidirectional_encoder():
    dims = dataclasses.replace(TINY, hidden=8)
    w = torch_ref.to_torch(synth.bidirectional_encoder_weights(9, dims), True, dtype=F64)
    seq, lens = _follower_inputs(10)[:2]
    r = np.random.default_rng(11)
    wts = [torch.tensor(r.standard_normal(s)) for s in ((B, T, dims.hidden), (B, dims.hidden), (B, dims.hidden))]
    d_ctx, d_emb = _mask(r, B, T, dims.hidden), _mask(r, B, T, dims.word)

    def f(enc):
        outs = torch_ref.encoder_bilstm(enc, torch.tensor(seq), lens, d_ctx, d_emb)
        return sum((o * m).sum() for o, m in zip(outs, wts))
    _gradcheck(f, w)
    ctx, h, c = torch_ref.encoder_bilstm(w, torch.tensor(seq), lens)
    for b, n in enumerate(lens):
        assert not ctx[b, n:].any()
    # one step each way: the one-token row's reverse half at position 0 is the reverse direction's only output
    Hd = dims.hidden // 2
    h1, c1 = torch_ref.lstm_cell(w['embedding.weight'][seq[3, :1]], torch.zeros(1, Hd, dtype=F64),
                                 torch.zeros(1, Hd, dtype=F64), *(w[k + '_reverse'] for k in (
                                     'lstm.weight_ih_l0', 'lstm.weight_hh_l0', 'lstm.bias_ih_l0', 'lstm.bias_hh_l0')))
    assert torch.equal(ctx[3, 0, Hd:], h1[0]) and torch.equal(c[3, :Hd], c1[0])


def _speaker_inputs(seed, Tp=3, words=4):
    r = np.random.default_rng(seed)
    acts = [r.standard_normal((B, TINY.feat)) for _ in range(Tp)]
    feats = [r.standard_normal((B, TINY.views, TINY.feat)) for _ in range(Tp)]
    pmask = np.zeros((B, Tp), bool)
    pmask[1, 2:] = True
    instr = r.integers(4, TINY.vocab, size=(B, words))
    instr[0, 2], instr[0, 3] = 2, 0                            # row 0: <EOS> then padding
    instr[2, 1:] = 0
    return acts, feats, torch.tensor(pmask), torch.tensor(instr)


@pytest.mark.parametrize('variant', ['glove', 'trainable', 'att_feed'])
def test_gradcheck_speaker_score_teacher_with_dropout(variant):
    senc_w, sdec_w = synth.speaker_weights(12, TINY)
    if variant == 'att_feed':
        sdec_w = synth.speaker_decoder_att_feed_weights(13, TINY)
    enc = torch_ref.to_torch(senc_w, True, dtype=F64)
    dec = torch_ref.to_torch(sdec_w, True, frozen=('embedding.weight',) if variant == 'glove' else (), dtype=F64)
    acts, feats, pmask, instr = _speaker_inputs(14)
    Tp, W = len(acts), instr.shape[1]
    r = np.random.default_rng(15)
    em = {t: _mask(r, B, 2 * TINY.feat) for t in range(Tp)}
    em['ctx'] = _mask(r, B, Tp, TINY.hidden)
    H, E = TINY.hidden, TINY.word
    if variant == 'att_feed':
        dm = [(None, _mask(r, B, H), _mask(r, B, H), _mask(r, B, 2 * H)) for _ in range(W)]
    else:
        dm = [(_mask(r, B, E) if variant == 'trainable' else None, _mask(r, B, H)) for _ in range(W)]

    def loss(e, d):
        return torch_ref.speaker_score(e, d, acts, feats, pmask, instr, W, 'teacher', enc_drop=em.__getitem__,
                                       dec_drop=dm.__getitem__)['loss']
    _gradcheck(lambda w: loss(enc, w), dec)
    _gradcheck(lambda w: loss(w, dec), enc)


# ---------------------------------------------------------------------------------------------- fp32 pins (goldens)

def _check_grads_sampled(got, g, prefix):
    """The goldens store a norm and 16 sampled entries per parameter; the fp32 oracle must reproduce them (norm to
    1e-4, entries to 1e-3: two fp32 evaluations in different summation orders)."""
    seen = 0
    gmax = max(float(v) for k, v in g.items() if k.startswith(prefix + 'gnorm/'))
    for name, t in got.items():
        key = prefix + 'gnorm/' + name
        if key not in g or t.grad is None:
            continue
        seen += 1
        flat = t.grad.detach().numpy().ravel()
        if g[key] < 1e-6 * gmax:            # shift-invariant biases: both hold their own roundoff of an exact zero
            assert np.sqrt(np.sum(flat.astype(np.float64) ** 2)) < 1e-5 * gmax, name
            continue
        np.testing.assert_allclose(np.sqrt(np.sum(flat.astype(np.float64) ** 2)), g[key], rtol=1e-4, atol=1e-9,
                                   err_msg=name)
        np.testing.assert_allclose(flat[g[prefix + 'gidx/' + name]], g[prefix + 'gval/' + name], rtol=1e-3,
                                   atol=1e-3 * g[key] / np.sqrt(flat.size) + 1e-9, err_msg=name)
    assert seen == sum(1 for k in g if k.startswith(prefix + 'gnorm/'))


def _follower_train_case(g, enc_w, dec_w, enc_seed_xor=0x5BD1E995):
    """make_golden_emb.py / make_golden_bidir.py: B 16, teacher forcing, this repo's masks at site0."""
    d = synth.FULL
    H, Fd, E = d.hidden, d.feat, d.word
    S_ = int(g['n_steps'])
    fb = synth.follower_batch(seed=int(g['batch_seed']), batch=16, steps=S_, n_viewpoints=64, min_len=5, max_len=20,
                              stop_prob=0.05)
    table = synth.feature_table(int(g['table_seed']), 64)
    seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, 80, reverse=True)
    Bn, Tn, rows, site0, seed = 16, max(lens), np.arange(16), int(g['site0']), int(g['dropout_seed'])
    Hc = enc_w['encoder2decoder.weight'].shape[0]
    seed_enc = seed ^ enc_seed_xor
    drop_emb = torch.tensor(orng.dropout_mask(seed_enc, site0 ^ 0x40000000, rows, 80 * E, 0.5).reshape(Bn, 80, E))

    def masks(t):
        if t == 'ctx':
            return torch.tensor(orng.dropout_mask(seed_enc, site0, rows, Tn * Hc, 0.5).reshape(Bn, Tn, Hc))
        return (torch.tensor(orng.dropout_mask(seed, 2 * (site0 + t), rows, 2 * Fd, 0.5)),
                torch.tensor(orng.dropout_mask(seed, 2 * (site0 + t) + 1, rows, H, 0.5)))
    enc = torch_ref.to_torch(enc_w, True)
    dec = torch_ref.to_torch(dec_w, True)
    loc = np_env.static_loc_embeddings()
    res = torch_ref.follower_rollout(enc, dec, torch.tensor(seq), lens, torch.tensor(mask), S_,
                                     lambda t: np_env.dense_follower_step(table, loc, fb, t), torch.tensor(fb.target),
                                     'teacher', Fd, drop_masks=masks, drop_emb=drop_emb)
    return enc, dec, res


def test_trainable_embedding_oracle_matches_g11(golden):
    g = golden('g11_follower_trainable_emb')
    enc_w, dec_w = synth.follower_weights_peaky(int(g['weight_seed']))
    enc, dec, res = _follower_train_case(g, enc_w, dec_w)
    want = g['logits_first']
    got = res['logits'][0].detach().numpy()[:, :want.shape[1]]
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=1e-4)
    np.testing.assert_allclose(res['loss'].item(), g['loss'], rtol=1e-5)
    res['loss'].backward()
    ge = enc['embedding.weight'].grad.numpy()
    assert float(np.abs(ge[0]).sum()) == 0.0
    assert int((np.abs(ge).sum(1) > 0).sum()) == int(g['emb_grad_rows_nonzero'])
    _check_grads_sampled(enc, g, 'enc/')
    _check_grads_sampled(dec, g, 'dec/')


def test_bidirectional_oracle_matches_g12(golden):
    g = golden('g12_encoder_bidir_eval')
    w = torch_ref.to_torch(synth.bidirectional_encoder_weights(int(g['weight_seed'])))
    lens = [int(x) for x in g['lengths']]
    ctx, h, c = torch_ref.encoder_bilstm(w, torch.tensor(g['seq']), lens)
    for name, got, want in (('ctx', ctx, g['ctx']), ('decoder_init', h, g['decoder_init']), ('c_t', c, g['c_t'])):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-5, atol=2e-6, err_msg=name)
    g = golden('g12_follower_bidir_train')
    enc_w = synth.bidirectional_encoder_weights(int(g['enc_weight_seed']))
    _, dec_w = synth.follower_weights_peaky(int(g['dec_weight_seed']))
    enc, dec, res = _follower_train_case(g, enc_w, dec_w)
    want = g['logits_first']
    got = res['logits'][0].detach().numpy()[:, :want.shape[1]]
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=1e-4)
    np.testing.assert_allclose(res['loss'].item(), g['loss'], rtol=1e-5)
    res['loss'].backward()
    _check_grads_sampled(enc, g, 'enc/')
    _check_grads_sampled(dec, g, 'dec/')


def test_att_feed_oracle_matches_g14(golden):
    g = golden('g14_speaker_att_feed')
    dec = torch_ref.to_torch(synth.speaker_decoder_att_feed_weights(int(g['weight_seed'])), True,
                             frozen=('embedding.weight',))
    ctx = torch.tensor(g['ctx'], requires_grad=True)
    h0 = torch.tensor(g['h0'], requires_grad=True)
    c0 = torch.tensor(g['c0'], requires_grad=True)
    mask = torch.tensor(g['mask'])
    h, c = h0, c0
    for t in range(3):
        h, c, alpha, logit = torch_ref.speaker_decoder_step_att_feed(dec, torch.tensor(g['words'][t]), h, c, ctx, mask)
        np.testing.assert_allclose(h.detach().numpy(), g['h1_%d' % t], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(c.detach().numpy(), g['c1_%d' % t], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(alpha.detach().numpy(), g['alpha_%d' % t], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(logit.detach().numpy(), g['logit_%d' % t], rtol=1e-5, atol=1e-5)
    ((logit * torch.tensor(g['g_logit'])).sum() + (h * torch.tensor(g['g_h'])).sum()).backward()
    _check_grads_sampled(dec, g, 'dec/')
    for name, t_ in (('d_h0', h0), ('d_c0', c0), ('d_ctx', ctx)):
        want = g[name]
        np.testing.assert_allclose(t_.grad.numpy(), want, rtol=1e-4, atol=1e-5 * float(np.abs(want).max()), err_msg=name)
