"""Oracle (test infrastructure): the hot path as differentiable torch-CPU functions,
so that autograd supplies the reference gradients for backward parity.  See
oracle/__init__.py for the rules.  Own code built from stock torch ops; each
function cites the reference lines it restates (paths under /root/reference).

Weights are dicts of torch tensors keyed like the reference state_dicts.  Every
function computes in the dtype of the weights it is given: fp32 by default
(`to_torch`), float64 with `to_torch(..., dtype=torch.float64)` -- the exact-arithmetic
anchor the training-gradient tests measure both the HIP path and the fp32 reference
against.  Inputs (features, masks) are cast to that dtype where they enter.
"""
import contextlib

import torch
import torch.nn.functional as F

# ---- rounded evaluation ---------------------------------------------------------------------------------------------
# Off by default.  Inside `rounded(...)` the result of every operator the oracle composes (linear, bmm, softmax, tanh,
# sigmoid, and the two sums of `lstm_cell`: the gate pre-activations and c_1) is rounded once to fp32 precision -- a model
# of a perfect implementation that stores every operator's result in fp32.  Run on float64 weights, the distance of such
# a run to the plain float64 one measures how far fp32 storage alone can move an output: the conditioning of the case.
_ROUND = None          # None | ('nearest', None) | ('random', torch.Generator)


@contextlib.contextmanager
def rounded(mode, generator=None):
    """mode 'nearest': x.float().double(); 'random': x * (1 + d), d uniform in +-2^-24 drawn from `generator`."""
    global _ROUND
    if mode not in ('nearest', 'random'):
        raise ValueError(mode)
    if mode == 'random' and generator is None:
        raise ValueError('random rounding needs a torch.Generator')
    prev, _ROUND = _ROUND, (mode, generator)
    try:
        yield
    finally:
        _ROUND = prev


def _r(x):
    if _ROUND is None:
        return x
    mode, gen = _ROUND
    if mode == 'nearest':
        return x.float().to(x.dtype)
    d = (torch.rand(x.shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * 2.0 ** -24
    return x * (1.0 + d).to(x.dtype)


def _linear(x, w, b=None):
    return _r(F.linear(x, w, b))


def _bmm(a, b):
    return _r(torch.bmm(a, b))


def _softmax(x, dim):
    return _r(torch.softmax(x, dim=dim))


def _tanh(x):
    return _r(torch.tanh(x))


def _sigmoid(x):
    return _r(torch.sigmoid(x))


def _rec(tape, name, value, per_step=True):
    """Record a named intermediate: appended to the list tape[name] (one entry per step), or stored as tape[name]."""
    if tape is None:
        return
    v = value.detach()
    if per_step:
        tape.setdefault(name, []).append(v)
    else:
        tape[name] = v


def to_torch(state, requires_grad=False, frozen=(), dtype=torch.float32):
    out = {}
    for k, v in state.items():
        t = torch.tensor(v, dtype=dtype)
        if requires_grad and k not in frozen:
            t.requires_grad_(True)
        out[k] = t
    return out


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh, tape=None):
    """nn.LSTMCell (gate order i,f,g,o) as used at model.py:393, 434, 515.  tape: records 'gates' (pre-activations) and
    'gates_act' (sigmoid / tanh applied: what the HIP cell keeps for its backward)."""
    gates = _r(_linear(x, w_ih, b_ih) + _linear(h, w_hh, b_hh))
    _rec(tape, 'gates', gates)
    i, f, g, o = gates.chunk(4, dim=1)
    sf = _sigmoid(f)
    si = _sigmoid(i)
    tg = _tanh(g)
    c1 = _r(sf * c + si * tg)
    so = _sigmoid(o)
    h1 = so * _tanh(c1)
    if tape is not None:
        _rec(tape, 'gates_act', torch.cat((si, sf, tg, so), 1))
    return h1, c1


def soft_dot_attention(h, context, mask, w_in, w_out):
    """model.py:122-143.  mask True = masked; filled on .data in the reference
    (:135), i.e. outside autograd -- masked_fill gives the same gradients."""
    target = _linear(h, w_in)
    attn = _bmm(context, target.unsqueeze(2)).squeeze(2)
    if mask is not None:
        attn = attn.masked_fill(mask, float('-inf'))
    attn = _softmax(attn, 1)
    weighted = _bmm(attn.unsqueeze(1), context).squeeze(1)
    h_tilde = _tanh(_linear(torch.cat((weighted, h), 1), w_out))
    return h_tilde, attn


def visual_soft_dot_attention(h, visual_context, w_h, b_h, w_v, b_v):
    """model.py:310-326."""
    target = _linear(h, w_h, b_h)
    context = _linear(visual_context, w_v, b_v)
    attn = _softmax(_bmm(context, target.unsqueeze(2)).squeeze(2), 1)
    weighted = _bmm(attn.unsqueeze(1), visual_context).squeeze(1)
    return weighted, attn


def eltwise_prod_scoring(h, all_u, w_h, b_h, w_a, b_a, w_out, b_out):
    """model.py:342-352."""
    target = _linear(h, w_h, b_h).unsqueeze(1)
    context = _linear(all_u, w_a, b_a)
    return _linear(target * context, w_out, b_out).squeeze(2)


def _lstm_over(enc, emb, lens, sfx, reverse=False):
    """One direction of the packed nn.LSTM (model.py:61-62, 89-90): rows advance over
    their own length only -- forward from position 0, reverse from position len-1
    down to 0 -- from a zero state (:68-79).  Returns (ctx [B,T,H] zero beyond a row's
    length, final h, final c)."""
    B, T = emb.shape[0], int(lens.max())
    H = enc['lstm.weight_hh_l0' + sfx].shape[1]
    h = torch.zeros(B, H, dtype=emb.dtype)
    c = torch.zeros(B, H, dtype=emb.dtype)
    outs = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        h1, c1 = lstm_cell(emb[:, t], h, c, enc['lstm.weight_ih_l0' + sfx], enc['lstm.weight_hh_l0' + sfx],
                           enc['lstm.bias_ih_l0' + sfx], enc['lstm.bias_hh_l0' + sfx])
        live = (t < lens).unsqueeze(1)
        h = torch.where(live, h1, h)
        c = torch.where(live, c1, c)
        outs[t] = torch.where(live, h1, torch.zeros_like(h1))
    return torch.stack(outs, dim=1), h, c


def _embed(enc, seq, drop_emb):
    """model.py:84-87: the embedded tokens, and -- trainable embedding (glove=None) in
    train mode -- their dropout; drop_emb: multiplicative mask [B, seq_len, E]."""
    emb = enc['embedding.weight'][seq]
    if drop_emb is not None:
        emb = emb * drop_emb.to(emb.dtype)
    return emb


def encoder_lstm(enc, seq, lengths, drop_ctx=None, drop_emb=None):
    """model.py:81-104 with packed-sequence semantics written out (rows stop
    advancing at their own length; ctx zero beyond).  drop_ctx: optional
    multiplicative mask for the ctx dropout at :102; drop_emb: the mask of the
    embedded tokens (:86-87, trainable embedding only; GloVe: no input dropout)."""
    emb = _embed(enc, seq, drop_emb)
    ctx, h, c = _lstm_over(enc, emb, torch.as_tensor(lengths), '')
    decoder_init = _tanh(_linear(h, enc['encoder2decoder.weight'], enc['encoder2decoder.bias']))
    if drop_ctx is not None:
        ctx = ctx * drop_ctx.to(ctx.dtype)
    return ctx, decoder_init, c


def encoder_bilstm(enc, seq, lengths, drop_ctx=None, drop_emb=None):
    """EncoderLSTM(bidirectional=True), model.py:47-66, 81-104: both directions over
    the packed sequence; ctx = [forward | reverse] per position (pad_packed_sequence,
    :101: zero beyond a row's length), h_t = cat(enc_h_t[-1], enc_h_t[-2]) -- the
    REVERSE direction's final state first (:93-94), c_t likewise, decoder_init =
    tanh(encoder2decoder(h_t)) (:99), then the ctx dropout (:102).  Masks as in
    `encoder_lstm` (drop_ctx over the assembled [B,T,2H])."""
    emb = _embed(enc, seq, drop_emb)
    lens = torch.as_tensor(lengths)
    ctx_f, h_f, c_f = _lstm_over(enc, emb, lens, '')
    ctx_r, h_r, c_r = _lstm_over(enc, emb, lens, '_reverse', reverse=True)
    ctx = torch.cat((ctx_f, ctx_r), 2)
    h_t = torch.cat((h_r, h_f), 1)
    c_t = torch.cat((c_r, c_f), 1)
    decoder_init = _tanh(_linear(h_t, enc['encoder2decoder.weight'], enc['encoder2decoder.bias']))
    if drop_ctx is not None:
        ctx = ctx * drop_ctx.to(ctx.dtype)
    return ctx, decoder_init, c_t


def attn_decoder_step(dec, u_prev, all_u, visual_context, h0, c0, ctx, ctx_mask,
                      drop_in=None, drop_h=None):
    """model.py:377-397."""
    p = 'visual_attention_layer.'
    feature, alpha_v = visual_soft_dot_attention(
        h0, visual_context, dec[p + 'linear_in_h.weight'], dec[p + 'linear_in_h.bias'],
        dec[p + 'linear_in_v.weight'], dec[p + 'linear_in_v.bias'])
    concat = torch.cat((u_prev, feature), 1)
    if drop_in is not None:
        concat = concat * drop_in
    h1, c1 = lstm_cell(concat, h0, c0, dec['lstm.weight_ih'], dec['lstm.weight_hh'],
                       dec['lstm.bias_ih'], dec['lstm.bias_hh'])
    h1_drop = h1 if drop_h is None else h1 * drop_h
    h_tilde, alpha = soft_dot_attention(
        h1_drop, ctx, ctx_mask, dec['text_attention_layer.linear_in.weight'],
        dec['text_attention_layer.linear_out.weight'])
    q = 'decoder2action.'
    logit = eltwise_prod_scoring(
        h_tilde, all_u, dec[q + 'linear_in_h.weight'], dec[q + 'linear_in_h.bias'],
        dec[q + 'linear_in_a.weight'], dec[q + 'linear_in_a.bias'],
        dec[q + 'linear_out.weight'], dec[q + 'linear_out.bias'])
    return h1, c1, alpha, logit, alpha_v


def follower_rollout(enc, dec, seq, lengths, ctx_mask, steps, step_inputs, targets,
                     feedback, dims_feat, drop_masks=None, drop_emb=None):
    """follower.py:430-539 without the simulator (see oracle.np_model.follower_rollout).
    drop_masks(t) -> (drop_in[B,2F], drop_h[B,H]) or None; drop_masks('ctx') -> [B,T,H].
    drop_emb: the embedded tokens' mask [B,seq_len,E] (trainable embedding, model.py:86-87).
    A bidirectional encoder (its state holds the `_reverse` weights) runs `encoder_bilstm`."""
    drop_ctx = drop_masks('ctx') if drop_masks else None
    encode = encoder_bilstm if 'lstm.weight_ih_l0_reverse' in enc else encoder_lstm
    ctx, h, c = encode(enc, seq, lengths, drop_ctx, drop_emb)
    dt = ctx.dtype
    B = seq.shape[0]
    u_prev = torch.zeros(B, dims_feat, dtype=dt)
    loss = torch.zeros((), dtype=dt)
    seq_scores = torch.zeros(B, dtype=dt)
    ended = torch.zeros(B, dtype=torch.bool)
    logits, actions = [], []
    for t in range(steps):
        X, all_u, is_valid = (torch.as_tensor(a) for a in step_inputs(t))
        X, all_u = X.to(dt), all_u.to(dt)
        d_in, d_h = drop_masks(t) if drop_masks else (None, None)
        h, c, alpha, logit, alpha_v = attn_decoder_step(dec, u_prev, all_u, X, h, c, ctx,
                                                        ctx_mask, d_in, d_h)
        logit = logit.masked_fill(is_valid == 0, float('-inf'))            # :477
        target = torch.where(ended, torch.full_like(targets[t], -1), targets[t])
        if bool((target != -1).any()):
            loss = loss + F.cross_entropy(logit, target, ignore_index=-1)  # :481
        if feedback == 'teacher':
            a_t = target.clamp(min=0)                                      # :486
        elif feedback == 'argmax':
            a_t = logit.argmax(dim=1)                                      # :488
        else:
            raise ValueError(feedback)
        u_prev = all_u[torch.arange(B), a_t].detach()                      # :502
        seq_scores = seq_scores - F.cross_entropy(logit, a_t, reduction='none').detach()
        logits.append(logit)
        actions.append(a_t)
        ended = ended | (a_t == 0)
        if bool(ended.all()):
            break
    return dict(logits=logits, actions=torch.stack(actions), loss=loss,
                scores=seq_scores, h=h, c=c, ctx=ctx)


def speaker_encoder(enc, action_embs, world_feats, drop_masks=None, tape=None):
    """model.py:437-457.  drop_masks(t) -> mask for the concat input (:433);
    drop_masks('ctx') -> mask for :456.  tape (a dict): per path step the lists 'alpha' (attention weights), 'feature'
    (attended feature), 'concat' (the masked LSTM input), 'gates', 'gates_act', 'h', 'c'; once 'decoder_init',
    'ctx_raw' and 'ctx' (the context before and after its mask)."""
    dt = enc['lstm.weight_hh'].dtype
    B = world_feats[0].shape[0]
    H = enc['lstm.weight_hh'].shape[1]
    h = torch.zeros(B, H, dtype=dt)
    c = torch.zeros(B, H, dtype=dt)
    hs = []
    p = 'visual_attention_layer.'
    for t, (a_emb, X) in enumerate(zip(action_embs, world_feats)):
        a_emb, X = torch.as_tensor(a_emb).to(dt), torch.as_tensor(X).to(dt)
        feature, alpha_v = visual_soft_dot_attention(
            h, X, enc[p + 'linear_in_h.weight'], enc[p + 'linear_in_h.bias'],
            enc[p + 'linear_in_v.weight'], enc[p + 'linear_in_v.bias'])
        concat = torch.cat((a_emb, feature), 1)
        if drop_masks:
            concat = concat * drop_masks(t).to(dt)
        _rec(tape, 'alpha', alpha_v)
        _rec(tape, 'feature', feature)
        _rec(tape, 'concat', concat)
        h, c = lstm_cell(concat, h, c, enc['lstm.weight_ih'], enc['lstm.weight_hh'],
                         enc['lstm.bias_ih'], enc['lstm.bias_hh'], tape)
        _rec(tape, 'h', h)
        _rec(tape, 'c', c)
        hs.append(h)
    decoder_init = _tanh(_linear(h, enc['encoder2decoder.weight'], enc['encoder2decoder.bias']))
    ctx = torch.stack(hs, dim=1)
    _rec(tape, 'decoder_init', decoder_init, False)
    _rec(tape, 'ctx_raw', ctx, False)
    if drop_masks:
        ctx = ctx * drop_masks('ctx').to(dt)
    _rec(tape, 'ctx', ctx, False)
    return ctx, decoder_init, c


def speaker_decoder_step(dec, prev_word, h0, c0, ctx, ctx_mask, drop_h=None, drop_emb=None):
    """model.py:497-519, the non-att-feed branch.  drop_emb: the mask of the embedded
    word (:499-500, trainable embedding only; GloVe: none); drop_h: dropout(h_1) (:516)."""
    emb = dec['embedding.weight'][prev_word]
    if drop_emb is not None:
        emb = emb * drop_emb.to(emb.dtype)
    h1, c1 = lstm_cell(emb, h0, c0, dec['lstm.weight_ih'], dec['lstm.weight_hh'],
                       dec['lstm.bias_ih'], dec['lstm.bias_hh'])
    h1_drop = h1 if drop_h is None else h1 * drop_h
    h_tilde, alpha = soft_dot_attention(
        h1_drop, ctx, ctx_mask, dec['attention_layer.linear_in.weight'],
        dec['attention_layer.linear_out.weight'])
    logit = _linear(h_tilde, dec['decoder2action.weight'], dec['decoder2action.bias'])
    return h1, c1, alpha, logit


def context_only_soft_dot_attention(h, context, mask, w_in, tape=None):
    """ContextOnlySoftDotAttention.forward, model.py:161-177.  tape: records 'target' (the linear_in output)."""
    target = _linear(h, w_in)
    _rec(tape, 'target', target)
    attn = _bmm(context, target.unsqueeze(2)).squeeze(2)
    if mask is not None:
        attn = attn.masked_fill(mask, float('-inf'))
    attn = _softmax(attn, 1)
    weighted = _bmm(attn.unsqueeze(1), context).squeeze(1)
    return weighted, attn


def speaker_decoder_step_att_feed(dec, prev_word, h0, c0, ctx, ctx_mask, drops=None, tape=None):
    """SpeakerDecoderLSTM.forward, the use_input_att_feed branch, model.py:497-513.
    drops: None (eval mode) or the four masks (embedded word [B,E] or None for GloVe,
    h_0 [B,H], h_tilde [B,H], cat(h_1, h_tilde) [B,2H]) of :500, :503, :504, :507.
    tape (a dict): appends this step's 'emb' (embedded word), 'h0_drop' (masked h_0), 'target' (linear_in output),
    'alpha' (attention weights), 'weighted' (weighted context), 'concat' (the masked LSTM input), 'gates', 'gates_act',
    'h1', 'c1', 'x_in' (the masked cat(h_1, h_tilde)), 'x' (the output_l1 tanh output) and 'logit' to the lists of those
    names."""
    d_emb, d_h0, d_ht, d_x = drops if drops is not None else (None, None, None, None)
    mul = lambda x, m: x if m is None else x * m.to(x.dtype)                # noqa: E731
    emb = mul(dec['embedding.weight'][prev_word], d_emb)                    # :497-500
    h0_drop = mul(h0, d_h0)
    _rec(tape, 'emb', emb)
    _rec(tape, 'h0_drop', h0_drop)
    h_tilde, alpha = context_only_soft_dot_attention(h0_drop, ctx, ctx_mask,
                                                     dec['attention_layer.linear_in.weight'], tape)  # :502-503
    concat = torch.cat((emb, mul(h_tilde, d_ht)), 1)                        # :504
    _rec(tape, 'alpha', alpha)
    _rec(tape, 'weighted', h_tilde)
    _rec(tape, 'concat', concat)
    h1, c1 = lstm_cell(concat, h0, c0, dec['lstm.weight_ih'], dec['lstm.weight_hh'],
                       dec['lstm.bias_ih'], dec['lstm.bias_hh'], tape)      # :505
    x_in = mul(torch.cat((h1, h_tilde), 1), d_x)                            # :506-507
    x = _tanh(_linear(x_in, dec['output_l1.weight'], dec['output_l1.bias']))   # :508-509
    logit = _linear(x, dec['decoder2action.weight'], dec['decoder2action.bias'])  # :510
    for name, v in (('h1', h1), ('c1', c1), ('x_in', x_in), ('x', x), ('logit', logit)):
        _rec(tape, name, v)
    return h1, c1, alpha, logit


def speaker_score(enc, dec, action_embs, world_feats, path_mask, instr_seq, steps,
                  feedback, pad_idx=0, bos_idx=3, eos_idx=2, enc_drop=None, dec_drop=None, tape=None):
    """speaker.py:135-197.  Train mode: enc_drop as `speaker_encoder`'s drop_masks;
    dec_drop(t) -> the masks of word step t: (drop_emb or None, drop_h) for the plain
    decoder, the four of `speaker_decoder_step_att_feed` for an att-feed decoder (its
    state holds `output_l1.weight`, model.py:475-481).  tape (a dict): filled with tape['enc'] (`speaker_encoder`'s
    tape) and, for an att-feed decoder, tape['dec'] (`speaker_decoder_step_att_feed`'s, one list entry per word step)."""
    enc_tape = dec_tape = None
    if tape is not None:
        enc_tape, dec_tape = tape.setdefault('enc', {}), tape.setdefault('dec', {})
    ctx, h, c = speaker_encoder(enc, action_embs, world_feats, enc_drop, enc_tape)
    dt = ctx.dtype
    att_feed = 'output_l1.weight' in dec
    B = ctx.shape[0]
    w_t = torch.full((B,), bos_idx, dtype=torch.long)
    ended = torch.zeros(B, dtype=torch.bool)
    loss = torch.zeros((), dtype=dt)
    seq_scores = torch.zeros(B, dtype=dt)
    words, logits = [], []
    for t in range(steps):
        if att_feed:
            h, c, alpha, logit = speaker_decoder_step_att_feed(
                dec, w_t, h, c, ctx, path_mask, dec_drop(t) if dec_drop else None, dec_tape)
        else:
            d_emb, d_h = dec_drop(t) if dec_drop else (None, None)
            h, c, alpha, logit = speaker_decoder_step(dec, w_t, h, c, ctx, path_mask, d_h, d_emb)
        target = instr_seq[:, t]
        if feedback == 'teacher':
            w_t = target
        elif feedback == 'argmax':
            w_t = logit.argmax(dim=1)
        else:
            raise ValueError(feedback)
        logp = F.log_softmax(logit, dim=1)
        seq_scores = seq_scores - F.nll_loss(logp, w_t, ignore_index=pad_idx,
                                             reduction='none').detach()
        if bool((target != pad_idx).any()):
            loss = loss + F.nll_loss(logp, target, ignore_index=pad_idx)
        logits.append(logit)
        words.append(w_t)
        ended = ended | (w_t == eos_idx)
        if bool(ended.all()):
            break
    return dict(logits=logits, words=torch.stack(words), loss=loss, scores=seq_scores,
                ctx=ctx, h=h, c=c)
