"""GPU: every element of the training gradients against float64 autograd.

Each case runs the forward and `loss.backward()` through the public engines (FollowerEngine.rollout /
SpeakerEngine.score, teacher forcing), feeds the identical inputs and the same counter-based dropout masks
(oracle/rng.py, at the sites the engine reports) to oracle/torch_ref.py in float64 and in fp32 on the CPU, and compares

  * the loss: relative 1e-5 to float64;
  * the logits of every step: 1e-4 absolute to float64 (finite entries; the -inf pattern identical); F6 alone (peaky
    weights, where the reference's own fp32 logits are 3.4e-4 from float64) is held to 4x that distance; S4 in train
    mode (the att-feed decoder, one ill-conditioned row) per (step, row) to max(1e-4, K x its conditioning envelope),
    tests/conditioning.py;
  * EVERY element of EVERY parameter's gradient with tests/grad_compare.py: e = max|g - r| / max|r| against
    e32 = max|f - r| / max|r| (the reference's own fp32 arithmetic), e <= max(4 e32, 2e-6) and e <= 1e-4, per tensor and
    per block (LSTM gates x input segments, the halves of the text attention's linear_out, every embedding row; rows
    zero by construction exactly zero);

and pins the path each case claims: from what the engine reports (enc.last_path / last_backward_path, st.teacher_path,
st.persistent, st.enc_table, st.wgrad_done_from), and where nothing reports it (the unidirectional encoder's launch,
gemm_tn_split) by repeating the pass with the path forced and comparing bits.  The CPU reference runs with torch's
thread count as the machine sets it; the module takes about 40 s on an MI355X host.  `-s` prints e / e32 of every tensor.

Measured on MI355X (worst tensor per case): default-scale weights (F1-F5, E2, S1-S6) e <= 1.4e-6 with e32 <= 2.0e-6;
S4 in train mode e <= 1.4e-5 (e32 9.2e-6); the trainable embedding (E1, peaky weights) e <= 1.6e-5 (e32 3.8e-5); G8's
peaky weights (F6) e <= 4.2e-4 with e32 4.5e-4 -- there the reference's own fp32 drift exceeds the 1e-4 ceiling, so F6
is held to 4 e32 alone.  Exact-zero biases: max|g| <= 3.0e-8, within 4x the fp32 reference's own roundoff of the zero.
Logits: <= 5.7e-6 from float64 everywhere except F6 (1.29e-4, the fp32 reference 3.36e-4) and the att-feed decoder in
train mode: 2.75e-4 at (step 8, row 0), 5.3e-5 at most in rows 1-11 (row 1: 4.6e-5).  That was this module's open
finding (a strict xfail: "2.75e-4 where the fp32 reference stays within 6.2e-5; rows 0-1") and is closed as CONDITIONING
OF ROW 0: rounding every operator's result once to fp32 in an otherwise float64 evaluation moves that entry by 3.8e-4
(the envelope), every stage of the HIP trace stays inside K x the envelope of the same stage, every operator alone is
within its fp32-class bound (tests/test_gpu_module_ladder.py), and the fp32 reference's 6.2e-5 was one lucky sample: the
same computation is 2.29e-4 away with 8 threads (tests/test_conditioning_host.py).  Row 1 is well-conditioned (envelope
2.3e-5), keeps the 1e-4 bound and is within it.  Numbers: profiles/att_feed_drift.txt.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_env, rng as orng, torch_ref                    # noqa: E402
from speaker_follower_amd import synth                                # noqa: E402
from tests import conditioning as cn                                  # noqa: E402
from tests import grad_compare as gc                                  # noqa: E402

D = synth.FULL
ENC_SEED_XOR = 0x5BD1E995           # FollowerEngine: encoder mask seed = seed ^ this
EMB_STREAM_XOR = 0x40000000         # include/sf_hip.h: SF_ENC_EMB_DROPOUT site = ctx site ^ this
SPK_ENC_SEED_XOR = 0x2545F491       # SpeakerEngine: encoder mask seed = seed ^ this
SEED = 4242


def _loc_segments(prefix=''):
    """Column segments of an LSTM input [x features | x location | attended features | attended location]."""
    I, L = D.img, D.loc
    return [(prefix + 'u_feat', 0, I), (prefix + 'u_loc', I, I + L), (prefix + 'att_feat', I + L, 2 * I + L),
            (prefix + 'att_loc', 2 * I + L, 2 * (I + L))]


def _lstm_blocks(state, pre, segs_ih=None):
    out = {}
    for k, v in state.items():
        if not k.startswith(pre):
            continue
        if '.weight_ih' in k:
            out[k] = gc.lstm_blocks(v.shape[0], segs_ih, cols=v.shape[1])
        elif '.weight_hh' in k:
            out[k] = gc.lstm_blocks(v.shape[0], cols=v.shape[1])
        elif '.bias_' in k:
            out[k] = gc.lstm_blocks(v.shape[0])
    return out


def _compare(tag, hip, r64, r32, blocks, ceiling=gc.CEILING):
    hip = {k: v for k, v in hip.items() if k in r64}
    assert set(hip) == set(r64), (tag, sorted(set(r64) ^ set(hip)))
    rep = gc.compare_grads(hip, r64, r32, blocks, what=tag, ceiling=ceiling)
    print('[grad] %s: worst tensor %s e = %.2e e32 = %.2e' % ((tag,) + rep.worst()))


def _check_logits(tag, got, ref64, ref32, n, fp32_relative=False):
    """1e-4 absolute to float64.  fp32_relative (peaky weights only, where the reference's own fp32 evaluation is itself
    further than 1e-4 from float64): within K times that distance."""
    worst = own = scale = 0.0
    for t in range(n):
        want = ref64[t].detach().numpy()
        g = got[t][:, :want.shape[1]]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(g), fin), '%s step %d: -inf pattern differs' % (tag, t)
        worst = max(worst, float(np.abs(g[fin] - want[fin]).max()))
        own = max(own, float(np.abs(ref32[t].detach().numpy()[fin] - want[fin]).max()))
        scale = max(scale, float(np.abs(want[fin]).max()))
    bound = max(1e-4, gc.K * own) if fp32_relative else 1e-4
    print('[parity] %s: max|dlogit| vs float64 over %d steps = %.3e, the fp32 reference %.3e, max|logit| %.2f '
          '(bound %.1e)' % (tag, n, worst, own, scale, bound))
    assert worst <= bound, (tag, worst, own)


def _grads(*mods):
    return {p_: {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None} for p_, m in mods}


def _same(a, b):
    """Bit-identical gradient sets."""
    return set(a) == set(b) and all(set(a[p]) == set(b[p]) and all(torch.equal(a[p][k], b[p][k]) for k in a[p])
                                    for p in a)


class _no_split:
    """The weight-gradient products on the fp32 MFMA kernels only (sf_debug_tn_split_min_rows): a pass that differs
    from the default one shows that the default took gemm_tn_split."""

    def __enter__(self):
        from speaker_follower_amd import _lib
        _lib.lib.sf_debug_tn_split_min_rows(1 << 30)

    def __exit__(self, *exc):
        from speaker_follower_amd import _lib
        _lib.lib.sf_debug_tn_split_min_rows(-1)


def _oracle_grads(state):
    return {k: v.grad for k, v in state.items() if v.grad is not None}


# --------------------------------------------------------------------------------------------------------- follower

def _follower(B, S, *, train, seed=11, weights='plain', glove=True, bidir=False, two_stream=True,
              persistent=True, min_len=10, max_len=79, a_max=14, stop_prob=1.0 / 6.0, mutate=None, max_length=80):
    from speaker_follower_amd import model, features, follower as fol
    if bidir:
        enc_w = synth.bidirectional_encoder_weights(seed)
        _, dec_w = synth.follower_weights(seed + 1)
        enc = model.EncoderLSTM(D.vocab, D.word, D.hidden // 2, 0, 0.5, bidirectional=True,
                                glove=enc_w['embedding.weight'] if glove else None)
    else:
        enc_w, dec_w = (synth.follower_weights_peaky if weights == 'peaky' else synth.follower_weights)(seed)
        enc = model.EncoderLSTM(D.vocab, D.word, D.hidden, 0, 0.5, glove=enc_w['embedding.weight'] if glove else None)
    dec = model.AttnDecoderLSTM(D.feat, D.hidden, 0.5, feature_size=D.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    enc.cuda().train(train)
    dec.cuda().train(train)
    enc.persistent = persistent
    fb = synth.follower_batch(seed=seed + 2, batch=B, steps=S, n_viewpoints=256, min_len=min_len, max_len=max_len,
                              a_max=a_max, stop_prob=stop_prob)
    if mutate:
        mutate(fb)
    table = synth.feature_table(seed + 3, 256)
    store = features.FeatureStore(table)
    batch = fol.DeviceFollowerBatch.from_synth(fb, max_length=max_length)

    def run(persistent=persistent, two_stream=two_stream):
        """One training pass through a fresh engine (same sites, same masks): (state, {enc/dec: gradients})."""
        for m in (enc, dec):
            m.zero_grad(set_to_none=True)
        enc.persistent = persistent
        eng = fol.FollowerEngine(enc, dec, store)
        eng.dropout_seed = SEED
        eng.two_stream_backward = two_stream
        st_ = eng.rollout(batch, S, 'teacher', train=train)
        st_.loss.backward()
        torch.cuda.synchronize()
        return st_, {pre: {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
                     for pre, m in (('enc', enc), ('dec', dec))}
    st, hip = run()
    logits = st.logits.detach().cpu().numpy()
    loss = float(st.loss.detach())

    seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, max_length, reverse=True)
    T, rows, site0 = max(lens), np.arange(B), st.site0
    loc = np_env.static_loc_embeddings()
    H, F, E = D.hidden, D.feat, D.word

    def masks(t):
        if t == 'ctx':
            return torch.tensor(orng.dropout_mask(SEED ^ ENC_SEED_XOR, site0, rows, T * H, 0.5).reshape(B, T, H))
        return (torch.tensor(orng.dropout_mask(SEED, 2 * (site0 + t), rows, 2 * F, 0.5)),
                torch.tensor(orng.dropout_mask(SEED, 2 * (site0 + t) + 1, rows, H, 0.5)))
    drop_emb = None
    if train and not glove:
        drop_emb = torch.tensor(orng.dropout_mask(SEED ^ ENC_SEED_XOR, site0 ^ EMB_STREAM_XOR, rows, max_length * E, 0.5)
                                .reshape(B, max_length, E))
    out = {}
    for dt in (torch.float64, torch.float32):
        e = torch_ref.to_torch(enc_w, True, frozen=('embedding.weight',) if glove else (), dtype=dt)
        d = torch_ref.to_torch(dec_w, True, dtype=dt)
        res = torch_ref.follower_rollout(e, d, torch.tensor(seq), lens, torch.tensor(mask), S,
                                         lambda t: np_env.dense_follower_step(table, loc, fb, t),
                                         torch.tensor(fb.target), 'teacher', F, drop_masks=masks if train else None,
                                         drop_emb=drop_emb)
        res['loss'].backward()
        out[dt] = (res, _oracle_grads(e), _oracle_grads(d))
    (r64, ge64, gd64), (r32, ge32, gd32) = out[torch.float64], out[torch.float32]
    n = len(r64['logits'])
    blocks = dict(_lstm_blocks(dec_w, 'lstm.', _loc_segments()))
    blocks['text_attention_layer.linear_out.weight'] = gc.halves_blocks(2 * H, H)
    eblocks = _lstm_blocks(enc_w, 'lstm.')
    if not glove:
        eblocks['embedding.weight'] = gc.row_blocks(D.vocab)
    return dict(st=st, enc=enc, dec=dec, hip=hip, run=run, logits=logits, loss=loss, r64=r64, r32=r32, n=n,
                g64=(ge64, gd64), g32=(ge32, gd32), blocks=(eblocks, blocks))


def _check_case(tag, c, ceiling=gc.CEILING, fp32_logits=False, logits=True):
    np.testing.assert_allclose(c['loss'], c['r64']['loss'].item(), rtol=1e-5, err_msg=tag)
    if logits:
        _check_logits(tag, c['logits'], c['r64']['logits'], c['r32']['logits'], c['n'], fp32_logits)
    _compare(tag + ' enc', c['hip']['enc'], c['g64'][0], c['g32'][0], c['blocks'][0], ceiling)
    _compare(tag + ' dec', c['hip']['dec'], c['g64'][1], c['g32'][1], c['blocks'][1], ceiling)


@pytest.mark.parametrize('two_stream', [True, False])
def test_f1_headline_training_shape(two_stream):
    """B 100, 20 steps, instructions of 10-79 tokens, train mode: the persistent encoder forward and backward (B <= 128),
    the stacked decoder weight gradients over 2000 rows (below gemm_tn_split's 4096), the deferred context gradient; BPTT
    on two streams and one.  sf_encoder_lstm_fwd does not report its path: the pass is repeated with the per-step encoder
    (SF_ENC_PER_STEP), whose context differs by roundoff -- so the default pass did run the persistent launch."""
    c = _follower(100, 20, train=True, two_stream=two_stream)
    assert c['st'].enc_table and c['n'] == 20
    _check_case('F1 two_stream=%s' % two_stream, c)
    st_ps, g_ps = c['run'](persistent=False)
    assert not torch.equal(st_ps.ctx, c['st'].ctx)


@pytest.mark.parametrize('B,S', [(256, 20), (300, 14)])
def test_f3_split_weight_gradient_and_unpaired_batches(B, S):
    """5120 / 4200 stacked rows: gemm_tn_split for the decoder weight gradients (pinned: the same pass with the split
    product switched off gives different bits); B > 128: the per-step encoder (pinned: forcing SF_ENC_PER_STEP changes
    no bit); B > 256: the un-paired launches.  B = 300 with the default two-stream backward failed with "workspace too
    small" in sf_follower_episode_bwd; above VIS_SPLIT_MAX_B (256) rows the entry now walks the steps on one stream (the
    two schedules give the same bits, so which one ran is not observable from the outputs)."""
    c = _follower(B, S, train=True, seed=31, min_len=5, max_len=40)
    assert B * c['n'] >= 4096
    _check_case('F3 B=%d S=%d' % (B, S), c)
    st_ps, g_ps = c['run'](persistent=False)
    assert torch.equal(st_ps.ctx, c['st'].ctx) and _same(g_ps, c['hip'])
    with _no_split():
        st_ns, g_ns = c['run']()
    assert not torch.equal(g_ns['dec']['lstm.weight_ih'], c['hip']['dec']['lstm.weight_ih'])


def test_f4_ragged_tiles_and_rows_that_end_at_step_zero():
    """Eval mode, B 37, 7 steps, instructions of 1-79 tokens, up to 16 candidates, frequent stops and rows whose first
    target is `stop` (they end at step 0 and carry no gradient afterwards).  Paths as F1 (persistent encoder, stacked
    products below the split's 4096 rows); not re-pinned here."""
    def mutate(fb):
        fb.target[0, :4] = np.where(fb.target[0, :4] >= 0, 0, fb.target[0, :4])
        fb.a_num[:, 5] = 16
    c = _follower(37, 7, train=False, seed=41, min_len=1, max_len=79, a_max=16, stop_prob=0.5, mutate=mutate)
    _check_case('F4 B=37 ragged', c)


def test_f5_smallest_shape():
    """B 1, 3 steps: the paths of F1 at one row (not re-pinned)."""
    c = _follower(1, 3, train=True, seed=51, min_len=3, max_len=12, stop_prob=0.0)
    _check_case('F5 B=1', c)


def test_f6_peaky_weights():
    """G8's peaky weights (O(1) logit spread): the reference's own fp32 drift is larger here, so the tensor bound is
    K x e32 (above the floor) without the 1e-4 ceiling, and the logits are held to K x the fp32 reference's distance.
    Measured: worst tensor e = 4.2e-4 (e32 4.5e-4, visual_attention_layer.linear_in_v.weight); logits 1.29e-4 from
    float64 where the fp32 reference is 3.36e-4 away (max |logit| 10.5)."""
    c = _follower(100, 20, train=True, seed=303, weights='peaky', stop_prob=1.0 / 40.0)
    _check_case('F6 peaky', c, ceiling=np.inf, fp32_logits=True)


def test_e1_trainable_embedding_with_embedding_dropout():
    """embedding_bwd with repeated tokens: every row of the table; the padding row and the rows of absent tokens
    exactly zero."""
    c = _follower(100, 10, train=True, seed=515, weights='peaky', glove=False)
    assert not c['st'].enc_table
    g = c['hip']['enc']['embedding.weight']
    assert float(g[0].abs().max()) == 0.0
    _check_case('E1 trainable embedding', c)


@pytest.mark.parametrize('persistent', [True, False])
@pytest.mark.parametrize('B', [64, 128])
def test_e2_bidirectional_encoder(B, persistent):
    c = _follower(B, 6, train=True, seed=9, bidir=True, persistent=persistent, min_len=1, max_len=79,
                  stop_prob=0.05)
    want = 'persistent' if persistent else 'per_step'
    assert c['enc'].last_path == want and c['enc'].last_backward_path == want
    _check_case('E2 bidirectional B=%d %s' % (B, want), c)


# ---------------------------------------------------------------------------------------------------------- speaker

def _speaker(B, S, *, train, seed=77, dims=D, glove=True, batched=True, stacked=True, att_feed=False, min_len=10,
             max_len=79, nvp=256):
    from speaker_follower_amd import model, features, speaker
    senc_w, sdec_w = synth.speaker_weights(seed, dims)
    if att_feed:
        sdec_w = synth.speaker_decoder_att_feed_weights(seed, dims)
    enc = model.SpeakerEncoderLSTM(dims.feat, dims.feat, dims.hidden, 0.5)
    dec = model.SpeakerDecoderLSTM(dims.vocab, dims.word, dims.hidden, 0.5,
                                   glove=sdec_w['embedding.weight'] if glove else None, use_input_att_feed=att_feed)
    enc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    enc.cuda().train(train)
    dec.cuda().train(train)
    sb = synth.speaker_batch(seed=seed + 1, batch=B, n_viewpoints=nvp, min_len=min_len, max_len=max_len, dims=dims)
    table = synth.feature_table(seed + 2, nvp)
    store = features.FeatureStore(table)
    batch = speaker.DeviceSpeakerBatch.from_synth(sb)
    se = SEED ^ SPK_ENC_SEED_XOR

    def run():
        """One pass through a fresh engine (same sites, same masks): (state, {enc/dec: gradients})."""
        for m in (enc, dec):
            m.zero_grad(set_to_none=True)
        # an att-feed decoder is stepped through the modules (SpeakerEngine._score_modules), whose dropout is keyed on
        # each module's own seed and call counter (model._DropState): start both at 0
        enc._drop_state.seed, enc._drop_state.counter = se, 0
        dec._drop_state.seed, dec._drop_state.counter = SEED, 0
        eng = speaker.SpeakerEngine(enc, dec, store)
        eng.dropout_seed = SEED
        eng.teacher_batched = batched
        eng.stacked_wgrad = stacked
        st_ = eng.score(batch, S, 'teacher', train=train)
        st_.loss.backward()
        torch.cuda.synchronize()
        return st_, _grads(('enc', enc), ('dec', dec))
    st, hip = run()
    logits = st.logits.detach().cpu().numpy()
    loss = float(st.loss.detach())

    acts, feats, path_mask = np_env.dense_speaker_inputs(sb, table, np_env.static_loc_embeddings())
    instr_seq, _, _ = np_env.batch_instructions_from_encoded(sb.instr, 80)
    Tp, rows, site0, H, F, E = len(acts), np.arange(B), st.site0, dims.hidden, dims.feat, dims.word
    assert Tp == batch.vp.shape[0]

    def enc_drop(t):
        if att_feed:          # module sites: path step t is the encoder's call t (2t), the context its call Tp (2Tp + 1)
            if t == 'ctx':
                return torch.tensor(orng.dropout_mask(se, 2 * Tp + 1, rows, Tp * H, 0.5).reshape(B, Tp, H))
            return torch.tensor(orng.dropout_mask(se, 2 * t, rows, 2 * F, 0.5))
        if t == 'ctx':
            return torch.tensor(orng.dropout_mask(se, 2 * (site0 + Tp) + 1, rows, Tp * H, 0.5).reshape(B, Tp, H))
        return torch.tensor(orng.dropout_mask(se, 2 * (site0 + t), rows, 2 * F, 0.5))

    def dec_drop(t):
        if att_feed:          # word step t is the decoder's call t: sites 4t + k (model.py:500, 503, 504, 507 order)
            return (None,) + tuple(torch.tensor(orng.dropout_mask(SEED, 4 * t + k, rows, n, 0.5))
                                   for k, n in ((1, H), (2, H), (3, 2 * H)))
        emb = None if glove else torch.tensor(orng.dropout_mask(SEED, 2 * (site0 + t), rows, E, 0.5))
        return emb, torch.tensor(orng.dropout_mask(SEED, 2 * (site0 + t) + 1, rows, H, 0.5))
    out = {}
    for dt in (torch.float64, torch.float32):
        e = torch_ref.to_torch(senc_w, True, dtype=dt)
        d = torch_ref.to_torch(sdec_w, True, frozen=('embedding.weight',) if glove else (), dtype=dt)
        res = torch_ref.speaker_score(e, d, acts, feats, torch.tensor(path_mask), torch.tensor(instr_seq), S,
                                      'teacher', enc_drop=enc_drop if train else None,
                                      dec_drop=dec_drop if train else None)
        res['loss'].backward()
        out[dt] = (res, _oracle_grads(e), _oracle_grads(d))
    (r64, ge64, gd64), (r32, ge32, gd32) = out[torch.float64], out[torch.float32]
    eblocks = _lstm_blocks(senc_w, 'lstm.', _loc_segments())
    dblocks = _lstm_blocks(sdec_w, 'lstm.', [('emb', 0, E), ('h_tilde', E, E + H)] if att_feed else None)
    if att_feed:
        dblocks['output_l1.weight'] = gc.halves_blocks(2 * H, H)           # [h_1 | h_tilde] (model.py:506)
    if 'attention_layer.linear_out.weight' in sdec_w:
        dblocks['attention_layer.linear_out.weight'] = gc.halves_blocks(2 * H, H)
    if not glove:
        dblocks['embedding.weight'] = gc.row_blocks(dims.vocab)
    return dict(st=st, enc=enc, dec=dec, hip=hip, run=run, logits=logits, loss=loss, r64=r64, r32=r32, n=len(r64['logits']),
                g64=(ge64, gd64), g32=(ge32, gd32), blocks=(eblocks, dblocks))


def test_s1_batched_teacher_backward():
    """B 100, 80 words, instructions of 10-79 tokens, train mode: the batched teacher pass and its backward, the
    weight gradients as one split product over 8000 rows (pinned: with the split product switched off the same pass
    gives different bits)."""
    c = _speaker(100, 80, train=True)
    assert c['st'].teacher_path and c['n'] == 80
    _check_case('S1 speaker batched teacher', c)
    with _no_split():
        st_ns, g_ns = c['run']()
    assert st_ns.teacher_path
    assert not torch.equal(g_ns['dec']['lstm.weight_hh'], c['hip']['dec']['lstm.weight_hh'])


def test_s2_word_loop_per_step_weight_gradients():
    c = _speaker(100, 80, train=True, batched=False, stacked=False)
    assert not c['st'].teacher_path and not c['st'].persistent
    _check_case('S2 speaker word loop, per-step wgrads', c)


def test_s3_trainable_speaker_embedding():
    """The embedding scatter per word step: every row; rows of absent words exactly zero."""
    c = _speaker(40, 32, train=True, glove=False, min_len=5, max_len=30)
    _check_case('S3 speaker trainable embedding', c)


@functools.lru_cache(maxsize=None)
def _s4(train):
    """The case and its references, computed once and shared by the two tests below (neither changes them)."""
    c = _speaker(12, 10, train=train, seed=31, att_feed=True, min_len=4, max_len=9, nvp=48)
    assert not c['st'].teacher_path and not c['st'].persistent
    if train:
        assert c['dec']._drop_state.counter == 10 and c['enc']._drop_state.counter == len(c['st'].batch.vp) + 1
    return c


@pytest.mark.parametrize('train', [False, True])
def test_s4_input_att_feed_decoder(train):
    """SpeakerDecoderLSTM(use_input_att_feed=True) (model.py:475-481, 500-513), which SpeakerEngine steps through the
    module's own forward (C-ABI operators under autograd), at the shape of tests/test_gpu_att_feed.py: B 12, 10 words.
    Train mode with the modules' counter-based masks (encoder: sites 2t / 2Tp + 1, decoder: 4t + k for the dropped h_0,
    h_tilde and cat(h_1, h_tilde)); the embedding is GloVe (a trainable one is refused on this path).  Loss and every
    gradient element in both modes; the logits in eval mode here (measured 5.6e-6 from float64, the fp32 reference
    9.6e-6), in train mode in the test below, per entry against the conditioning envelope."""
    c = _s4(train)
    _check_case('S4 att-feed %s' % ('train' if train else 'eval'), c, logits=not train)


def test_s4_att_feed_train_logits_within_envelope_of_float64():
    """Every (step, row) of the train-mode logits within max(1e-4, K x env) of float64, env the conditioning envelope of
    that entry (tests/conditioning.py: the float64 oracle with every operator's result rounded once to fp32, 1 nearest + 32
    seeded random roundings; computed once per process).  The earlier yardstick, one fp32 evaluation of the reference,
    is printed beside it: it is a single sample whose value depends on the host's thread count
    (tests/test_conditioning_host.py).  No entry is skipped; the -inf pattern must be identical."""
    c = _s4(True)
    case = cn.s4(True)
    env, _ = cn.s4_envelope(True)
    bound = cn.entry_bounds(env)
    ref = case.run()
    n = c['n']
    assert n == len(ref) == env.shape[0] == 10 and env.shape[1] == 12
    for t in range(n):                          # the envelope's float64 run IS this module's float64 reference
        assert torch.equal(ref[t], c['r64']['logits'][t].detach())
    got = [c['logits'][t][:, :ref[t].shape[1]] for t in range(n)]
    for t in range(n):
        assert got[t].shape == tuple(ref[t].shape)
        assert np.array_equal(np.isfinite(got[t]), np.isfinite(ref[t].numpy())), 'step %d: -inf pattern differs' % t
    d = cn.logit_distance(got, ref)
    d32 = cn.logit_distance(c['r32']['logits'], ref)
    assert d.shape == bound.shape
    ratio = d / bound
    t_, r_ = np.unravel_index(np.argmax(ratio), ratio.shape)
    plain = bound == cn.ABS_BOUND
    dp = np.where(plain, d, -1.0)
    tp, rp = np.unravel_index(np.argmax(dp), dp.shape)
    ta, ra = np.unravel_index(np.argmax(d), d.shape)
    print('[parity] S4 att-feed train: worst entry by ratio (step %d, row %d): |dlogit| %.3e, env %.3e, bound %.3e, '
          'ratio %.2f' % (t_, r_, d[t_, r_], env[t_, r_], bound[t_, r_], ratio[t_, r_]))
    print('[parity] S4 att-feed train: largest |dlogit| %.3e at (step %d, row %d), env there %.3e' % (d[ta, ra], ta, ra,
                                                                                                      env[ta, ra]))
    print('[parity] S4 att-feed train: worst entry among the %d of %d pairs whose bound is 1e-4 (step %d, row %d): '
          '|dlogit| %.3e, env %.3e' % (plain.sum(), plain.size, tp, rp, d[tp, rp], env[tp, rp]))
    print('[parity] S4 att-feed train: per-row max |dlogit| %s' % ['%.2e' % v for v in d.max(0)])
    print('[parity] S4 att-feed train: the fp32 reference on this host (%d threads): %.3e from float64 at (step %d, row '
          '%d)' % ((torch.get_num_threads(), d32.max()) + np.unravel_index(np.argmax(d32), d32.shape)))
    bad = ['(step %d, row %d): %.3e > %.3e (env %.3e)' % (t, r, d[t, r], bound[t, r], env[t, r])
           for t, r in zip(*np.nonzero(d > bound))]
    assert not bad, 'S4 att-feed train logits outside max(1e-4, K env): ' + '; '.join(bad)


def test_s5_vocabulary_above_1024():
    d = dataclasses.replace(D, vocab=1086)
    c = _speaker(12, 14, train=True, seed=31, dims=d, min_len=4, max_len=12, nvp=48)
    assert not c['st'].persistent
    _check_case('S5 speaker vocab 1086', c)


def test_s6_smallest_shape():
    c = _speaker(1, 8, train=True, seed=61, min_len=3, max_len=6, nvp=48)
    _check_case('S6 speaker B=1', c)
