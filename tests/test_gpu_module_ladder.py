"""GPU: the operator ladder of the att-feed speaker's module path (SpeakerEngine._score_modules), S4 shape (B 12, path of 6
steps, 10 words, vocab 991), train and eval mode.

tests/test_gpu_grads_f64.py holds the END of this path (loss, logits, gradients) to float64; every kernel on it is held
alone elsewhere.  What was missing is the path in between: which operator, at which step, an end-to-end distance comes
from.  Three rungs:

(a) The trace is the engine's.  A hand-written loop over the module-level callables the engine composes
    (_AttnLstmStepFn, _dropout_apply, linear, _TextAttnFn, lstm_cell, sf_gather_rows, _PaddedLinearFn), same seeds and
    call counters, records every intermediate the oracle's tape names (oracle/torch_ref.py); its logits equal
    `eng.score(...).logits` bit for bit.  (The HIP cell keeps its gates ACTIVATED -- the tape's 'gates_act'; the
    pre-activations never reach memory.  In train mode the fused encoder step never materialises the unmasked attended
    feature either: the HIP tape has it in eval mode only, the masked concat in both.)

(b) Local accuracy.  For every stage and step the float64 tape's inputs to that stage, rounded to fp32, are given to the
    HIP operator; its result g is compared with the same operator in float64 on the same inputs (r) and with stock torch
    in fp32 on the CPU (f).  The LSTM cell's gate product never reaches memory on its own: it is launched alone on the
    same inputs through sf_linear_slabs_fwd (the one launch the cell makes; its split-K slabs summed in float64), and
    the cell as a whole (activated gates, c_1, h_1) is held by the rule below.  The cell behind the visual attention of
    the fused _AttnLstmStepFn is judged on the input it actually consumed: that operator's own masked concat.
      products (LSTM gates at K 4864 + 512 and E + H + 512, linear_in, output_l1, decoder2action at width 991 through
      the padded path, encoder2decoder):   |g - r| <= 2.5e-7 * sum |a| |b|   per element (bias terms included);
      both attentions' weights and weighted sums, the cell, the tanh epilogues:  the grad_compare rule,
      e = max|g - r| / max|r| <= max(K * e32, FLOOR) and <= CEILING with e32 the same for f;
      dropout copies and the embedding gather: exactly oracle.rng.dropout_mask times the input / the table's rows.

(c) Free-running trace (a report, no assertion): the HIP tape of (a) against the float64 tape, entry by entry and per
    (step, row), beside the conditioning envelope of the same tape entry (tests/conditioning.py); the first stage and
    step at which any row leaves K * env is named.  (The envelope models fp32 STORAGE of every operator's result, not
    fp32 accumulation inside a product: in eval mode, where nothing is amplified, a few entries sit at 1.0-1.2 x K env at
    the 1e-7 level -- accumulation roundoff, which (b) bounds.  In train mode no entry of any stage leaves K env.)

`-s` prints e / e32 of every stage and the report.  Measured on MI355X (profiles/att_feed_drift.txt): products at most
9.1e-8 of sum |a| |b| (bound 2.5e-7; torch's fp32 product 1.4e-7); rule stages e <= 5.6e-7 with e32 <= 2.7e-6; every
dropout copy and gather exact; train-mode trace: worst d / (K env) 0.91 (the decoder's activated gates, step 7), logits
0.61.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import rng as orng, torch_ref                             # noqa: E402
from tests import conditioning as cn                                  # noqa: E402
from tests import grad_compare as gc                                  # noqa: E402

PRODUCT = 2.5e-7            # per-element bound of an fp32-class product, x sum |a| |b| (tests/test_gpu_gate_rows.py)
BOS = 3
SE = cn.SEED ^ cn.SPK_ENC_SEED_XOR


@functools.lru_cache(maxsize=None)
def _world(train):
    """Modules, feature store and device batch of tests/test_gpu_grads_f64.py::_s4, and the oracle's side of it."""
    from speaker_follower_amd import model, features, speaker
    case = cn.s4(train)
    d = case.dims
    enc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    dec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=case.sdec_w['embedding.weight'],
                                   use_input_att_feed=True)
    enc.load_state_dict({k: torch.tensor(v) for k, v in case.senc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in case.sdec_w.items()})
    enc.cuda().train(train)
    dec.cuda().train(train)
    store = features.FeatureStore(case.table)
    batch = speaker.DeviceSpeakerBatch.from_synth(case.sb)
    env, tenv = cn.s4_envelope(train)
    return dict(case=case, enc=enc, dec=dec, store=store, batch=batch, env=env, tenv=tenv, t64=tenv['f64'])


def _engine_inputs(w):
    """The dense inputs of the module API as SpeakerEngine._score_modules forms them."""
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    store, batch = w['store'], w['batch']
    Tp, B, Fd = batch.vp.shape[0], batch.batch_size, store.F
    act = torch.empty(Tp, B, Fd, device=store.device)
    call('sf_gather_path_actions', ptr(store.table), store.V, store.IMG, store.LOC, ptr(batch.vp), ptr(batch.act_view),
         ptr(batch.act_sincos), ptr(batch.act), Tp * B, ptr(act), Fd, stream())
    live = (batch.vp >= 0)
    feats = [store.gather_panorama(batch.vp[t].clamp(min=0), batch.view[t]) * live[t].view(B, 1, 1).float()
             for t in range(Tp)]
    return [act[t] for t in range(Tp)], feats


def _enc_step(enc, cfg, a_emb, X, h, c):
    """_AttnLstmStepFn and what it saved: (h1, c1, masked concat, attention weights, activated gates)."""
    from speaker_follower_amd import model as M
    from speaker_follower_amd.runtime import f32
    h1, c1 = M._AttnLstmStepFn.apply(enc, cfg, f32(a_emb), f32(X), h.contiguous(), c.contiguous(), *enc._params8())
    _, _, _, xin, alpha, _, _, gates = h1.grad_fn.saved_tensors
    return h1, c1, xin, alpha, gates


def _hip_trace(w):
    """(a): the engine's module path, written out over the module-level callables; returns the tape (CPU, float64)."""
    from speaker_follower_amd import model as M, ops
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    case, enc, dec, batch = w['case'], w['enc'], w['dec'], w['batch']
    train = case.train
    B, S, Tp, Fd, E = case.B, case.S, case.Tp, case.dims.feat, case.dims.word
    assert Tp == batch.vp.shape[0]
    te, td = {}, {}
    rec = lambda tp, k, v: tp.setdefault(k, []).append(v.detach().cpu().double())   # noqa: E731
    acts, feats = _engine_inputs(w)
    h, c = enc.init_state(B)
    hs = []
    for t in range(Tp):                                              # SpeakerEncoderLSTM.forward
        cfg = (0.5, SE, t) if train else (0.0, 0, 0)
        h, c, xin, alpha, gates = _enc_step(enc, cfg, acts[t], feats[t], h, c)
        rec(te, 'alpha', alpha)
        if not train:
            rec(te, 'feature', xin[:, Fd:])
        for k, v in (('concat', xin), ('gates_act', gates), ('h', h), ('c', c)):
            rec(te, k, v)
        hs.append(h)
    dinit = M.linear(enc.encoder2decoder, h, act=1)
    ctx = torch.stack(hs, dim=1)
    te['ctx_raw'] = ctx.detach().cpu().double()
    if train:
        ctx = M._dropout_apply(ctx, 0.5, SE, 2 * Tp + 1)
    te['ctx'], te['decoder_init'] = ctx.detach().cpu().double(), dinit.detach().cpu().double()
    h = dinit
    mask = ops.mask_u8(batch.path_mask)
    logits = []
    for t in range(S):                                               # SpeakerDecoderLSTM._forward_att_feed, teacher forcing
        words = torch.full((B,), BOS, dtype=torch.int64, device=h.device) if t == 0 else batch.instr_seq[:, t - 1]
        drop = (lambda x, k: M._dropout_apply(x, 0.5, cn.SEED, 4 * t + k)) if train else (lambda x, k: x)
        emb = torch.empty(B, E, device=h.device, dtype=torch.float32)
        call('sf_gather_rows', ptr(dec.embedding.weight.detach()), E, ptr(words.to(torch.int32).contiguous()), B, E,
             ptr(emb), E, stream())
        h0d = drop(h, 1)
        tq = M.linear(dec.attention_layer.linear_in, h0d)
        wc, alpha = M._TextAttnFn.apply(tq, ctx.contiguous(), mask)
        concat = torch.cat((emb, drop(wc, 2)), 1)
        h1, c1 = M.lstm_cell(dec.lstm, concat, h, c)
        gates = h1.grad_fn.saved_tensors[4]
        x_in = drop(torch.cat((h1, wc), 1), 3)
        x = M.linear(dec.output_l1, x_in, act=1)
        assert dec.decoder2action.weight.shape[0] % 4
        logit = M._PaddedLinearFn.apply(dec.decoder2action, x.contiguous(), dec.decoder2action.weight,
                                        dec.decoder2action.bias)
        for k, v in (('emb', emb), ('h0_drop', h0d), ('target', tq), ('alpha', alpha), ('weighted', wc), ('concat', concat),
                     ('gates_act', gates), ('h1', h1), ('c1', c1), ('x_in', x_in), ('x', x), ('logit', logit)):
            rec(td, k, v)
        logits.append(logit.detach())
        h, c = h1, c1
    return {'enc': te, 'dec': td}, torch.stack(logits)


@functools.lru_cache(maxsize=None)
def _traced(train):
    w = _world(train)
    from speaker_follower_amd import speaker
    enc, dec = w['enc'], w['dec']
    enc._drop_state.seed, enc._drop_state.counter = SE, 0
    dec._drop_state.seed, dec._drop_state.counter = cn.SEED, 0
    eng = speaker.SpeakerEngine(enc, dec, w['store'])
    eng.dropout_seed = cn.SEED
    st = eng.score(w['batch'], w['case'].S, 'teacher', train=train)
    tape, logits = _hip_trace(w)
    torch.cuda.synchronize()
    return st.logits.detach().clone(), tape, logits


@pytest.mark.parametrize('train', [False, True])
def test_a_hand_written_loop_is_the_engine(train):
    eng_logits, tape, logits = _traced(train)
    assert eng_logits.shape == logits.shape == (10, 12, 991)
    assert torch.equal(eng_logits, logits)
    assert all(torch.equal(tape['dec']['logit'][t], logits[t].cpu().double()) for t in range(10))


# ---------------------------------------------------------------------------------------------------- (b) local accuracy

class _Table:
    def __init__(self):
        self.rows, self.bad = {}, []

    def add(self, stage, step, e, e32, ok, what):
        r = self.rows.setdefault(stage, [0.0, 0.0, -1, what])
        if e >= r[0]:
            r[0], r[2] = e, step
        r[1] = max(r[1], e32)
        if not ok:
            self.bad.append('%s step %d: %s e = %.3e (e32 = %.3e)' % (stage, step, what, e, e32))

    def show(self, tag):
        print()
        for stage, (e, e32, step, what) in self.rows.items():
            print('[ladder] %s %-24s %-9s worst e = %.2e (step %d)  e32 = %.2e' % (tag, stage, what, e, step, e32))


def _product(tb, stage, step, got, terms, biases=()):
    """got [M,N] (device) against sum_i x_i w_i^T + sum biases in float64: per element 2.5e-7 * sum |a| |b|; e printed
    as the worst ratio |g - r| / sum|a||b| (so the bound is e <= 2.5e-7), e32 likewise for torch's fp32 product."""
    r = sum(x.double() @ wt.double().t() for x, wt in terms)
    mag = sum(x.double().abs() @ wt.double().abs().t() for x, wt in terms)
    f = sum(F.linear(x.float(), wt.float()) for x, wt in terms)
    for b in biases:
        r, mag, f = r + b.double(), mag + b.double().abs(), f + b.float()
    g = got.detach().cpu().double()
    assert g.shape == r.shape, (stage, g.shape, r.shape)
    e = float(((g - r).abs() / mag).max())
    e32 = float(((f.double() - r).abs() / mag).max())
    tb.add(stage, step, e, e32, bool(torch.isfinite(g).all()) and e <= PRODUCT, 'product')
    return r


def _rule(tb, stage, step, got, r, f):
    """The grad_compare rule relative to max|r|."""
    g = got.detach().cpu().double()
    assert g.shape == r.shape == f.shape, (stage, g.shape, r.shape, f.shape)
    scale = float(r.abs().max())
    e = float((g - r).abs().max()) / scale
    e32 = float((f.double() - r).abs().max()) / scale
    ok = bool(torch.isfinite(g).all()) and e <= max(gc.K * e32, gc.FLOOR) and e <= gc.CEILING
    tb.add(stage, step, e, e32, ok, 'rule')


def _exact(tb, stage, step, got, want):
    g = got.detach().cpu()
    tb.add(stage, step, float((g.double() - want.double()).abs().max()), 0.0, torch.equal(g, want.float()), 'exact')


def _cell(gates, c0):
    """The pointwise half of nn.LSTMCell on pre-activations: (activated gates, c1, h1)."""
    i, f, g, o = gates.chunk(4, dim=1)
    act = torch.cat((torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)), 1)
    si, sf, tg, so = act.chunk(4, dim=1)
    c1 = sf * c0 + si * tg
    return act, c1, so * torch.tanh(c1)


def _gate_product(cell, x, h):
    """The cell's gate product alone, x W_ih^T + h W_hh^T without the biases (sf_linear_slabs_fwd: the one launch
    sf_lstm_cell_fwd makes for it), its split-K slabs summed in float64: [M, 4H] on the CPU."""
    import ctypes as C
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, ws_args, workspace
    xd, hd = x.float().cuda().contiguous(), h.float().cuda().contiguous()
    M, K1, K2, N = xd.shape[0], xd.shape[1], hd.shape[1], cell.weight_ih.shape[0]
    ks = C.c_int(0)
    call('sf_linear_slabs_fwd', ptr(xd), K1, ptr(cell.weight_ih.detach()), K1, ptr(hd), K2, ptr(cell.weight_hh.detach()),
         K2, M, N, C.byref(ks), *ws_args(xd.device))
    torch.cuda.synchronize()
    assert 1 <= ks.value <= 64
    slabs = workspace(xd.device).view(torch.float32)[:ks.value * M * N].view(ks.value, M, N)
    return slabs.double().sum(0).cpu()


def _cell_stage(tb, part, t, cell, w32, pre, x, h0, c0, gates, c1, h1):
    """x, h0, c0: the cell's fp32 inputs (CPU); gates, c1, h1: what the HIP cell made of them."""
    terms = [(x, w32[pre + 'weight_ih']), (h0, w32[pre + 'weight_hh'])]
    r = _product(tb, part + '.gates', t, _gate_product(cell, x, h0), terms)
    b64 = w32[pre + 'bias_ih'].double() + w32[pre + 'bias_hh'].double()
    ar, cr, hr = _cell(r + b64, c0.double())
    af, cf, hf = _cell(F.linear(x, w32[pre + 'weight_ih'], w32[pre + 'bias_ih']) +
                       F.linear(h0, w32[pre + 'weight_hh'], w32[pre + 'bias_hh']), c0)
    names = ('gates_act', 'c', 'h') if part == 'enc' else ('gates_act', 'c1', 'h1')
    for name, g, r_, f_ in zip(names, (gates, c1, h1), (ar, cr, hr), (af, cf, hf)):
        _rule(tb, '%s.%s' % (part, name), t, g, r_, f_)


def _mask(seed, site, B, n):
    return torch.tensor(orng.dropout_mask(seed, site, np.arange(B), n, 0.5))


@pytest.mark.parametrize('train', [False, True])
def test_b_every_operator_alone_on_the_float64_tape(train):
    from speaker_follower_amd import model as M, ops
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    w = _world(train)
    case, enc, dec, batch = w['case'], w['enc'], w['dec'], w['batch']
    B, S, Tp, Fd, E, H = case.B, case.S, case.Tp, case.dims.feat, case.dims.word, case.dims.hidden
    t64 = w['t64']
    f32_of = lambda v: v.float()                                      # noqa: E731  (the stage's input, rounded once)
    dev = lambda v: v.float().cuda().contiguous()                     # noqa: E731
    e64, d64 = case.weights(torch.float64)
    e32, d32 = case.weights(torch.float32)
    tb = _Table()
    acts, feats = _engine_inputs(w)
    p = 'visual_attention_layer.'
    vis = lambda wd, h, X: torch_ref.visual_soft_dot_attention(       # noqa: E731
        h, X, wd[p + 'linear_in_h.weight'], wd[p + 'linear_in_h.bias'], wd[p + 'linear_in_v.weight'],
        wd[p + 'linear_in_v.bias'])
    with torch.no_grad():
        zero = torch.zeros(B, H)
        for t in range(Tp):                                          # ---- encoder: the fused step
            h0 = f32_of(t64[('enc', 'h')][t - 1]) if t else zero
            c0 = f32_of(t64[('enc', 'c')][t - 1]) if t else zero
            a, X = acts[t].cpu(), feats[t].cpu()
            cfg = (0.5, SE, t) if train else (0.0, 0, 0)
            with torch.enable_grad():
                h1, c1, xin, alpha, gates = _enc_step(enc, cfg, acts[t], feats[t], dev(h0), dev(c0))
            m = _mask(SE, 2 * t, B, 2 * Fd) if train else torch.ones(B, 2 * Fd)
            feat_r, alpha_r = vis(e64, h0.double(), X.double())
            feat_f, alpha_f = vis(e32, h0, X)
            _rule(tb, 'enc.alpha', t, alpha, alpha_r, alpha_f)
            _rule(tb, 'enc.feature', t, xin[:, Fd:], feat_r * m[:, Fd:].double(), feat_f * m[:, Fd:])
            _exact(tb, 'enc.concat[action]', t, xin[:, :Fd], a * m[:, :Fd])
            _cell_stage(tb, 'enc', t, enc.lstm, e32, 'lstm.', xin.detach().cpu(), h0, c0, gates, c1, h1)
        hT = f32_of(t64[('enc', 'h')][Tp - 1])                       # ---- encoder2decoder, the context's mask
        pre = M.linear(enc.encoder2decoder, dev(hT), act=0)
        r = _product(tb, 'encoder2decoder', 0, pre, [(hT, e32['encoder2decoder.weight'])], [e32['encoder2decoder.bias']])
        _rule(tb, 'decoder_init', 0, M.linear(enc.encoder2decoder, dev(hT), act=1), torch.tanh(r),
              torch.tanh(F.linear(hT, e32['encoder2decoder.weight'], e32['encoder2decoder.bias'])))
        ctx_raw = torch.stack([f32_of(v) for v in t64[('enc', 'ctx_raw')]], 1)
        if train:
            _exact(tb, 'enc.ctx[mask]', 0, M._dropout_apply(dev(ctx_raw), 0.5, SE, 2 * Tp + 1),
                   ctx_raw * _mask(SE, 2 * Tp + 1, B, Tp * H).reshape(B, Tp, H))
        ctx = torch.stack([f32_of(v) for v in t64[('enc', 'ctx')]], 1)
        ctx_d, mask_d = dev(ctx), ops.mask_u8(batch.path_mask)
        pmask = torch.tensor(case.path_mask)
        assert torch.equal(batch.path_mask.cpu().bool(), pmask)
        w_in = 'attention_layer.linear_in.weight'
        for t in range(S):                                           # ---- decoder, one word step
            D = {k: f32_of(t64[('dec', k)][t])
                 for k in ('emb', 'h0_drop', 'target', 'weighted', 'concat', 'h1', 'x_in', 'x')}
            h0 = f32_of(t64[('dec', 'h1')][t - 1] if t else t64[('enc', 'decoder_init')][0])
            c0 = f32_of(t64[('dec', 'c1')][t - 1] if t else t64[('enc', 'c')][Tp - 1])
            words = torch.full((B,), BOS, dtype=torch.int64) if t == 0 else torch.tensor(case.instr_seq[:, t - 1])
            emb = torch.empty(B, E, device='cuda')
            call('sf_gather_rows', ptr(dec.embedding.weight.detach()), E, ptr(words.to(torch.int32).cuda()), B, E,
                 ptr(emb), E, stream())
            _exact(tb, 'dec.emb', t, emb, d32['embedding.weight'][words])
            if train:
                for k, src, n, name in ((1, h0, H, 'dec.h0_drop'), (2, D['weighted'], H, 'dec.concat[mask]'),
                                        (3, torch.cat((D['h1'], D['weighted']), 1), 2 * H, 'dec.x_in')):
                    _exact(tb, name, t, M._dropout_apply(dev(src), 0.5, cn.SEED, 4 * t + k),
                           src * _mask(cn.SEED, 4 * t + k, B, n))
            _product(tb, 'dec.linear_in', t, M.linear(dec.attention_layer.linear_in, dev(D['h0_drop'])),
                     [(D['h0_drop'], d32[w_in])])
            wc, alpha = M._TextAttnFn.apply(dev(D['target']), ctx_d, mask_d)
            # (the oracle's attention from its linear_in OUTPUT: an identity weight leaves the rounded target as it is)
            eye64, eye32 = torch.eye(H, dtype=torch.float64), torch.eye(H)
            wr, ar = torch_ref.context_only_soft_dot_attention(D['target'].double(), ctx.double(), pmask, eye64)
            wf, af = torch_ref.context_only_soft_dot_attention(D['target'], ctx, pmask, eye32)
            assert not alpha.cpu()[pmask].any() and not ar[pmask].any()
            _rule(tb, 'dec.alpha', t, alpha, ar, af)
            _rule(tb, 'dec.weighted', t, wc, wr, wf)
            with torch.enable_grad():
                h1, c1 = M.lstm_cell(dec.lstm, dev(D['concat']), dev(h0), dev(c0))
                gates = h1.grad_fn.saved_tensors[4]
            _cell_stage(tb, 'dec', t, dec.lstm, d32, 'lstm.', D['concat'], h0, c0, gates, c1, h1)
            pre = M.linear(dec.output_l1, dev(D['x_in']), act=0)
            r = _product(tb, 'dec.output_l1', t, pre, [(D['x_in'], d32['output_l1.weight'])], [d32['output_l1.bias']])
            _rule(tb, 'dec.x', t, M.linear(dec.output_l1, dev(D['x_in']), act=1), torch.tanh(r),
                  torch.tanh(F.linear(D['x_in'], d32['output_l1.weight'], d32['output_l1.bias'])))
            assert dec.decoder2action.weight.shape[0] == 991
            logit = M._PaddedLinearFn.apply(dec.decoder2action, dev(D['x']), dec.decoder2action.weight,
                                            dec.decoder2action.bias)
            _product(tb, 'dec.decoder2action', t, logit, [(D['x'], d32['decoder2action.weight'])],
                     [d32['decoder2action.bias']])
    tb.show('train' if train else 'eval')
    want = {'enc.alpha', 'enc.feature', 'enc.concat[action]', 'enc.gates', 'enc.gates_act', 'enc.c', 'enc.h',
            'encoder2decoder', 'decoder_init', 'dec.emb', 'dec.linear_in', 'dec.alpha', 'dec.weighted', 'dec.gates',
            'dec.gates_act', 'dec.c1', 'dec.h1',
            'dec.output_l1', 'dec.x', 'dec.decoder2action'}
    if train:
        want |= {'enc.ctx[mask]', 'dec.h0_drop', 'dec.concat[mask]', 'dec.x_in'}
    assert set(tb.rows) == want
    assert not tb.bad, '\n'.join(tb.bad)


# ---------------------------------------------------------------------------------------------- (c) free-running report

ORDER = [('enc', k) for k in ('alpha', 'feature', 'concat', 'gates', 'gates_act', 'c', 'h', 'ctx_raw', 'ctx',
                              'decoder_init')] + \
        [('dec', k) for k in ('emb', 'h0_drop', 'target', 'alpha', 'weighted', 'concat', 'gates', 'gates_act', 'c1', 'h1',
                              'x_in', 'x', 'logit')]
NOT_IN_MEMORY = {('enc', 'gates'), ('dec', 'gates')}       # the HIP cell keeps its gates activated only


@pytest.mark.parametrize('train', [False, True])
def test_c_free_running_trace_report(train):
    """A report: where the free-running HIP trace first leaves K x the envelope of the same tape entry.  The assertions
    are (b) and tests/test_gpu_grads_f64.py::test_s4_att_feed_train_logits_within_envelope_of_float64; here only the
    tape's completeness is asserted."""
    w = _world(train)
    _, tape, _ = _traced(train)
    hip = cn.tape_entries(tape)
    t64, tenv = w['t64'], w['tenv']
    assert set(t64) == set(ORDER)
    assert set(hip) == set(ORDER) - NOT_IN_MEMORY - ({('enc', 'feature')} if train else set())
    tag = 'train' if train else 'eval'
    print()
    Tp, S = w['case'].Tp, w['case'].S
    once = ('ctx_raw', 'ctx', 'decoder_init')
    walk = [(k, t) for t in range(Tp) for k in ORDER if k[0] == 'enc' and k[1] not in once]
    walk += [(('enc', n), t) for n in once[:2] for t in range(Tp)] + [(('enc', 'decoder_init'), 0)]
    walk += [(k, t) for t in range(S) for k in ORDER if k[0] == 'dec']
    first = None
    for key, t in walk:                                              # in the order the path computes them
        if key not in hip:
            continue
        d = cn.tape_distance({key: hip[key][t:t + 1]}, {key: t64[key][t:t + 1]})[key][0]
        out = d > gc.K * tenv[key][t]
        if out.any():
            r = int(np.argmax(np.where(out, d / np.maximum(gc.K * tenv[key][t], 1e-300), 0)))
            first = (key, t, r, d[r], tenv[key][t, r])
            break
    for key in ORDER:
        if key not in hip:
            continue
        d = cn.tape_distance({key: hip[key]}, {key: t64[key]})[key]
        env = tenv[key]
        scale = max(float(v.abs().max()) for v in t64[key])
        t_, r_ = np.unravel_index(np.argmax(d), d.shape)
        ratio = np.where(d > 0, d / np.maximum(gc.K * env, 1e-300), 0.0)
        tr, rr = np.unravel_index(np.argmax(ratio), ratio.shape)
        print('[trace] %s %-18s max|x| %.2e  worst |hip - f64| %.2e (step %d, row %d; env there %.2e)  worst '
              'd / (K env) %.2f (step %d, row %d)  entries outside %d of %d'
              % (tag, '.'.join(key), scale, d[t_, r_], t_, r_, env[t_, r_], ratio[tr, rr], tr, rr,
                 int((d > gc.K * env).sum()), d.size))
    if first is None:
        print('[trace] %s: no tape entry leaves K x its envelope' % tag)
    else:
        print('[trace] %s: first outside K x envelope: %s step %d row %d, |hip - f64| %.3e, env %.3e'
              % ((tag, '.'.join(first[0])) + first[1:]))
