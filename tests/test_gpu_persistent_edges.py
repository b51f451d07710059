"""The persistent launches of csrc/sf_persist.hip -- the speaker's word loop (spk_persist_kernel<false|true>), the
encoder's recurrence (enc_persist_kernel<1|2>, also as the teacher-forced speaker's recurrence with an initial state) and
its backward (enc_bwd_persist_kernel<1|2>) -- one launch at a time, at every edge of their partition (tests/persist_cases.py:
the tables, the inputs, the float64 models; tests/test_persist_cases_host.py checks those on the host, and shows that the
comparator refuses what an off-by-one in the partition would hand back).

The entries are called directly.  Every output buffer is NaN-filled (integers: a sentinel) with three guard rows behind
the last row, the logits tape with its padding columns [vocab, ldv): the guards must come back untouched.  After every
launch the workspace's fault word is read and must be 0 ("starved launch": a launch that gave up a bounded wait poisons its
outputs, which must not pass for a numeric failure), and _lib.kernel_profile() must name the persistent kernel (the
refusals and the fall-back: must not).

Word loop: the float64 model is fed the words the launch emitted, every step stands alone.  Per tensor
e = max |gpu - r64| / max |r64| against e32, the same figure of the float32 evaluation of the same model;
e <= max(4 e32, 2e-6) and e <= 1e-4 (tests/grad_compare.py).  Teacher feedback: the words are the targets.  Argmax: the
emitted word's float64 logit lies within 2 x bound of the float64 maximum, and IS the arg max wherever the float64 top-2
margin exceeds 2 x bound.  Passing NULL for the optional tapes, and launching again, give the same bits.

Measured on an MI355X (the case with the largest e of each group as (e, e32); `-s` prints every figure):
    word loop  teacher  plain   logits (4.6e-07, 6.5e-07)  alpha (2.6e-07, 2.0e-07)  h1 (2.4e-07, 2.3e-07)  c1 (1.8e-07, 1.6e-07)
                                step_scores (1.9e-07, 1.1e-07)  nll_term (1.9e-07, 1.1e-07)
    word loop  teacher  peaky   logits (2.2e-06, 8.6e-06)  alpha (2.2e-06, 1.7e-06)  h1 (2.2e-07, 3.7e-07)  c1 (1.7e-07, 3.4e-07)
                                step_scores (8.1e-07, 1.8e-06)  nll_term (8.1e-07, 1.8e-06)
    word loop  argmax   plain   logits (4.6e-07, 4.8e-07)  alpha (2.6e-07, 2.1e-07)  h1 (3.0e-07, 2.0e-07)  c1 (3.5e-07, 1.6e-07)
                                step_scores (2.0e-07, 1.2e-07)  nll_term (1.9e-07, 8.3e-08)
    word loop  argmax   peaky   logits (2.8e-06, 1.5e-05)  alpha (2.7e-06, 1.4e-05)  h1 (2.6e-07, 4.8e-07)  c1 (1.9e-07, 2.8e-07)
                                step_scores (1.5e-05, 3.5e-05)  nll_term (1.1e-06, 3.0e-06)
    word loop  sample   peaky   logits (3.1e-06, 2.0e-06)  alpha (2.7e-06, 1.8e-06)  h1 (4.1e-07, 3.1e-07)  c1 (3.3e-07, 3.3e-07)
                                step_scores (2.5e-06, 2.8e-06)  nll_term (2.0e-06, 6.2e-06)
    teacher recurrence          logits (3.0e-07, 4.3e-07)  alpha (1.2e-07, 3.4e-07)  h1 (1.9e-07, 2.0e-07)  c1 (1.1e-07, 1.8e-07)
                                step_scores (1.7e-07, 8.2e-08)  nll_term (1.7e-07, 8.2e-08)
    encoder forward, eval       ctx (3.0e-07, 3.0e-07)  h (2.5e-07, 3.4e-07)  c (2.9e-07, 3.6e-07)  gates (3.2e-07, 4.1e-07)
                                hs (3.0e-07, 3.0e-07)  cs (2.9e-07, 3.7e-07)
    encoder forward, train      ctx (2.9e-07, 2.9e-07); the other tensors as in eval mode
    encoder backward            dgates (1.6e-07, 1.8e-07); bidirectional: forward (1.5e-07, 2.5e-07), reverse (2.9e-07, 4.5e-07)
                                weight gradients: the largest e 4.6e-07 (encoder2decoder.weight at B 128, T 3; e32 6.0e-07)
The largest share of a bound any tensor used is 0.45 (logits, vocab 1024, peaky, argmax): no case has a bound of its own.
Argmax: the float64 margin was clear at every (step, row) of 39 cases and at 0.998 of them in one; every emitted word was
the float64 arg max there.  Sample: all 36 draws of each vocabulary were clear and equal to the mirror's.

Found by the first run: the backward step added dctx of positions beyond a row's length to dh (all three forms: the
persistent launch's forward direction, lstm_bwd_step_fused_kernel, lstm_pw_bwd_elem); a dead step passes dh on, so it
reached the row's last live step -- dgates off by 0.39 .. 4.0 of their scale under the random dctx of these cases, invisible
in training, where the text attention hands zeros there.  Fixed in the kernels; test_dctx_beyond_a_length_reaches_nothing
pins it for the persistent and the per-step path.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rng as orng, torch_ref                             # noqa: E402
from speaker_follower_amd import synth                                # noqa: E402
from tests import grad_compare as GC                                  # noqa: E402
from tests import persist_cases as PC                                 # noqa: E402

GUARD = 3
WORD_SENTINEL, ENDED_SENTINEL = -7, 0xCC
PAD, EOS, BOS = PC.PAD, PC.EOS, PC.BOS
FEEDBACK = dict(teacher=0, argmax=1, sample=2)
H, E = PC.H, PC.E


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """A device buffer of `shape` filled with NaN (floats) or a sentinel, with GUARD rows of the last dimension behind it."""

    def __init__(self, *shape, dtype=torch.float32, fill=float('nan')):
        n = int(np.prod(shape))
        self.fill = fill
        self.full = torch.full((n + GUARD * shape[-1],), fill, dtype=dtype, device='cuda')
        self.t = self.full[:n].view(*shape)

    def ptr(self):
        return C.c_void_p(self.full.data_ptr())

    def untouched(self, whole=False):
        tail = self.full if whole else self.full[self.t.numel():]
        return bool(torch.isnan(tail).all()) if self.fill != self.fill else bool((tail == self.fill).all())

    def np(self):
        return self.t.cpu().numpy()


def no_fault(what):
    from speaker_follower_amd import runtime
    torch.cuda.synchronize()
    bits = runtime.take_fault(torch.device('cuda', torch.cuda.current_device()))
    assert bits == 0, '%s: starved launch (fault bits %d): the outputs are poisoned, not wrong' % (what, bits)


def persistent_kernels(prof):
    return sorted(k for k in prof.rows if 'persist_kernel' in k)


# ---------------------------------------------------------------------------------- speaker word loop
@functools.lru_cache(maxsize=2)
def decoder_module(vocab, peaky, tie=None):
    from speaker_follower_amd import model
    w = PC.speaker_decoder_weights(vocab, peaky)
    if tie is not None:
        w = PC.tie_weights(w, tie)
    dec = model.SpeakerDecoderLSTM(vocab, E, H, 0.5, glove=w['embedding.weight'])
    dec.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return dec.cuda().eval(), w


def decode(dec, case, inp, feedback, sample=None, tapes=True):
    """sf_speaker_decode on guarded buffers: (status, outputs as numpy, guards, persistent kernels that ran)."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import ptr, ws_args
    V, Tp, B, S = case.vocab, case.Tp, case.B, case.S
    ldv = PC.ldv(V)
    g = dict(words=Guarded(S + 1, B, dtype=torch.int64, fill=WORD_SENTINEL),
             ended=Guarded(B, dtype=torch.uint8, fill=ENDED_SENTINEL),
             step_scores=Guarded(S, B), nll_term=Guarded(S, B), live=Guarded(S, B),
             logits=Guarded(S, B, ldv), alpha=Guarded(S, B, Tp), h1=Guarded(S, B, H), c1=Guarded(S, B, H))
    g['words'].t[0] = BOS
    g['ended'].t.zero_()
    ins = [dev(a) for a in (inp.targets, inp.h_init, inp.c_init, inp.ctx, inp.mask)]
    w = dec._w_struct(table=True)
    opt = [g[k].ptr() if tapes else None for k in ('logits', 'alpha', 'h1', 'c1')]
    with _lib.kernel_profile() as prof:
        rc = _lib.lib.sf_speaker_decode(C.byref(w), B, H, Tp, V, S, FEEDBACK[feedback], PAD, EOS, *(ptr(x) for x in ins),
                                        g['words'].ptr(), g['ended'].ptr(), g['step_scores'].ptr(), g['nll_term'].ptr(),
                                        g['live'].ptr(), *opt, C.byref(sample) if sample is not None else None,
                                        *ws_args(torch.device('cuda')))
        torch.cuda.synchronize()
    no_fault('sf_speaker_decode %s %s' % (case, feedback))
    out = {k: v.np() for k, v in g.items()}
    out['logits_pad'] = out['logits'][..., V:]
    out['logits'] = out['logits'][..., :V]
    return rc, out, g, persistent_kernels(prof)


def guards_untouched(g, tapes=True):
    for k, v in g.items():
        assert v.untouched(whole=not tapes and k in ('logits', 'alpha', 'h1', 'c1')), 'guard rows of %s were written' % k


EXACT = ('words', 'ended', 'step_scores', 'nll_term', 'live')
ROWS = []                                   # (what, tensor, e, e32, bound) of every comparison of the session


def check_word_loop(case, feedback, dec, dec_w, inp, sample=None, kernel=PC.SPK_KERNEL, named=None):
    """One launch against the float64 model fed the launch's own words; then the same launch without its optional
    outputs and once more with them: the same bits.  Returns (outputs, float64 model, float32 model)."""
    what = 'v%d Tp%d%s B%d S%d %s %s' % (case.vocab, case.Tp, '' if case.mask else ' nomask', case.B, case.S,
                                         'peaky' if case.peaky else 'plain', feedback)
    rc, out, g, ran = decode(dec, case, inp, feedback, sample)
    assert rc == 0 and ran == [kernel], (rc, ran)
    guards_untouched(g)
    assert np.isnan(out['logits_pad']).all(), 'the padding columns [vocab, ldv) of the logits tape were written'
    words = out['words']
    assert (words[0] == BOS).all() and words.min() >= 0 and words.max() < case.vocab
    for k in PC.TENSORS:
        assert np.isfinite(out[k]).all(), '%s: %s holds non-finite values' % (what, k)
    r64 = PC.word_loop(dec_w, inp, words)
    r32 = PC.word_loop(dec_w, inp, words, torch.float32)
    PC.compare(what, out, r64, r32, PC.TENSORS, named=named, rows=ROWS)
    PC.check_exact_flags(out, r64, words)
    PC.check_alpha(out['alpha'], inp.mask)
    rc2, bare, g2, ran2 = decode(dec, case, inp, feedback, sample, tapes=False)
    assert rc2 == 0 and ran2 == [kernel]
    guards_untouched(g2, tapes=False)
    for k in EXACT:
        assert np.array_equal(bare[k], out[k], equal_nan=True), 'without the optional outputs %s differs' % k
    rc3, again, g3, _ = decode(dec, case, inp, feedback, sample)
    assert rc3 == 0
    for k in EXACT + PC.TENSORS:
        assert np.array_equal(again[k], out[k], equal_nan=True), 'the same launch twice: %s differs' % k
    return out, r64, r32


def _id(case):
    return 'v%d-Tp%d%s-B%d-S%d%s' % (case.vocab, case.Tp, '' if case.mask else 'n', case.B, case.S, '-peaky' if case.peaky else '')


@pytest.mark.parametrize('feedback', PC.FEEDBACKS)
@pytest.mark.parametrize('case', PC.SPEAKER, ids=_id)
def test_word_loop_against_float64_at_every_edge(case, feedback):
    dec, dec_w = decoder_module(case.vocab, case.peaky)
    inp = PC.speaker_inputs(case)
    out, r64, r32 = check_word_loop(case, feedback, dec, dec_w, inp)
    if feedback == 'teacher':
        assert np.array_equal(out['words'][1:], inp.targets)
    else:
        clear = PC.check_argmax_words(out['words'], r64['logits'], PC.logit_bound_abs(r64, r32))
        print('[persist] argmax: %.3f of the (step, row) pairs have a clear float64 margin' % clear)


@pytest.mark.parametrize('vocab,pair', PC.TIES, ids=lambda x: str(x).replace(' ', ''))
def test_a_tie_of_the_arg_max_goes_to_the_lower_index(vocab, pair):
    """Two columns with identical decoder2action rows and biases, the clear maximum: their logits are bit-equal (every
    column goes through the same operation sequence -- if a later kernel breaks that, rework this test), and argmax
    emits the lower index at every step and row, whichever thread, lane, workgroup or merge lane holds the other."""
    case = PC._spk(vocab=vocab, B=PC.TIE_B, S=PC.TIE_S)
    dec, dec_w = decoder_module(vocab, False, pair)
    inp = PC.speaker_inputs(case)
    rc, out, g, ran = decode(dec, case, inp, 'argmax')
    assert rc == 0 and ran == [PC.SPK_KERNEL]
    guards_untouched(g)
    lo, hi = (np.ascontiguousarray(out['logits'][..., c]) for c in pair)
    assert np.array_equal(lo.view(np.int32), hi.view(np.int32)), 'the tied columns do not hold the same bits'
    rest = np.delete(out['logits'], list(pair), axis=2)
    assert float((lo - rest.max(2)).min()) > 10.0                      # the clear maximum
    PC.check_tie_words(out['words'], pair)
    # score = log p(word): two columns share nearly all the mass
    np.testing.assert_allclose(out['step_scores'], -np.log(np.exp(out['logits'].astype(np.float64) - lo[..., None]).sum(2)),
                               rtol=0, atol=1e-5)


@pytest.mark.parametrize('vocab', PC.SAMPLE_VOCABS)
def test_sample_feedback_draws_the_mirrors_words(vocab):
    """spk_persist_kernel<true>: every word equals oracle.rng.speaker_sample on the launch's own logits of that step
    wherever its margin exceeds 1e-5; words lie in [0, vocab) (empty slots carry mass 0 and are never drawn); scores equal
    log p(word) -- through the float64 model fed the sampled words, under the rule."""
    from speaker_follower_amd import _lib
    case = PC._spk(vocab=vocab, peaky=True)
    dec, dec_w = decoder_module(vocab, True)
    inp = PC.speaker_inputs(case)
    seed, stream, row0 = 0x2F6E2B1, 17, 300
    smp = _lib.Sample(seed, stream, row0, None)
    out, r64, r32 = check_word_loop(case, 'sample', dec, dec_w, inp, sample=smp, kernel=PC.SPK_SAMPLE_KERNEL)
    words, logits = out['words'], out['logits']
    n_clear = n_all = 0
    for t in range(case.S):
        u1, u2 = orng.sample_uniforms(seed, stream + t, row0 + np.arange(case.B))
        for b in range(case.B):
            w, margin = orng.speaker_sample(logits[t, b], u1[b], u2[b])
            n_all += 1
            if margin > 1e-5:
                n_clear += 1
                assert words[t + 1, b] == w, (t, b, words[t + 1, b], w, margin)
    print('[persist] sample v%d: %d of %d draws clear' % (vocab, n_clear, n_all))
    assert n_clear > 0.98 * n_all
    lse = np.log(np.exp(logits.astype(np.float64) - logits.max(2, keepdims=True)).sum(2)) + logits.max(2)
    pick = np.take_along_axis(logits, words[1:, :, None], axis=2)[:, :, 0]
    np.testing.assert_allclose(out['step_scores'], np.where(words[1:] != PAD, pick - lse, 0.0), rtol=1e-4, atol=2e-4)


@pytest.mark.parametrize('r', PC.REFUSALS, ids=lambda r: r.what.replace(' ', '_'))
def test_one_step_past_each_limit_is_refused_and_nothing_is_written(r):
    case = PC.Spk(r.vocab, r.Tp, r.B, 4, True, False)
    dec, dec_w = decoder_module(r.vocab, False)
    inp = PC.speaker_inputs(case)
    rc, out, g, ran = decode(dec, case, inp, {v: k for k, v in FEEDBACK.items()}[r.feedback])
    assert rc == r.status and ran == [], (rc, ran)
    for k, v in g.items():
        if k == 'words':
            assert (v.t[0] == BOS).all() and (v.full[r.B:] == WORD_SENTINEL).all()
        elif k == 'ended':
            assert not v.t.any() and v.untouched()
        else:
            assert v.untouched(whole=True), k


@pytest.mark.parametrize('vocab,persistent', [(935, True), (PC.VOCAB_MAX + 1, False)])
def test_the_engine_takes_the_launch_where_it_applies(vocab, persistent):
    """SpeakerEngine.score at the second live vocabulary and one word past the limit: st.persistent, and the words of the
    per-step path either way."""
    import dataclasses
    from speaker_follower_amd import model, features, speaker
    d = dataclasses.replace(synth.FULL, vocab=vocab)
    senc_w, sdec_w = synth.speaker_weights_peaky(31, d)
    enc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    dec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    enc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    enc.cuda().eval()
    dec.cuda().eval()
    B, S, NVP = 9, 6, 48
    sb = synth.speaker_batch(seed=9, batch=B, n_viewpoints=NVP, min_path=3, max_path=5, min_len=3, max_len=S - 1, dims=d)
    store = features.FeatureStore(synth.feature_table(7, NVP))
    batch = speaker.DeviceSpeakerBatch.from_synth(sb)
    got = {}
    for allowed in (True, False):
        eng = speaker.SpeakerEngine(enc, dec, store)
        eng.persistent = allowed
        with torch.no_grad():
            st = eng.score(batch, S, 'argmax', train=False)
        no_fault('SpeakerEngine.score')
        assert st.persistent == (allowed and persistent)
        got[allowed] = st.words.cpu().numpy()
    assert np.array_equal(got[True], got[False])


# ------------------------------------------------------------------------------------ encoder forward
@functools.lru_cache(maxsize=2)
def encoder_module(bidir=False, seed=101):
    from speaker_follower_amd import model
    d = synth.FULL
    w = synth.bidirectional_encoder_weights(seed) if bidir else synth.follower_weights(seed)[0]
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden // (2 if bidir else 1), 0, 0.5, bidirectional=bidir,
                            glove=w['embedding.weight'])
    enc.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return enc.cuda(), w


DROP = (0.5, 0xBEEF, 3)                     # p, seed, row0; the stream (site) is 7
SITE = 7
ENC_KEYS = ('ctx', 'h', 'c', 'gates', 'hs', 'cs')


def drop_mask(train, B, width):
    return orng.dropout_mask(DROP[1], SITE, DROP[2] + np.arange(B), width, DROP[0]) if train else None


def encoder_fwd(enc, seq, lens, persistent, train):
    """sf_encoder_lstm_fwd on guarded buffers: (guarded buffers, persistent kernels that ran)."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.model import _encoder_structs
    from speaker_follower_amd.runtime import ptr, ws_args, dropout_arg
    enc.persistent = persistent
    try:
        B, Lpad = seq.shape
        T = max(lens)
        g = dict(ctx=Guarded(B, T, H), h=Guarded(B, H), c=Guarded(B, H), emb=Guarded(T, B, E), xg=Guarded(T, B, 4 * H),
                 gates=Guarded(T, B, 4 * H), hs=Guarded(T + 1, B, H), cs=Guarded(T + 1, B, H))
        tp = _lib.EncoderTape(*(g[k].full.data_ptr() for k in ('emb', 'xg', 'gates', 'hs', 'cs')))
        w = _encoder_structs(enc)
        lens_dev = torch.tensor(lens, dtype=torch.int32, device='cuda')
        with _lib.kernel_profile() as prof:
            _lib.call('sf_encoder_lstm_fwd', C.byref(w), B, Lpad, T, E, H, ptr(seq), ptr(lens_dev), g['ctx'].ptr(), g['h'].ptr(),
                      g['c'].ptr(), C.byref(tp), dropout_arg(*(DROP if train else (0.0, 0))), SITE, *ws_args(seq.device))
            torch.cuda.synchronize()
    finally:
        enc.persistent = True
    no_fault('sf_encoder_lstm_fwd B=%d T=%d' % (B, T))
    return g, persistent_kernels(prof)


def model_tensors(m, d='f'):
    n = lambda t: t.detach().double().numpy()                  # noqa: E731
    return dict(ctx=n(m['ctx']), h=n(m['decoder_init']), c=n(m['c_t']), gates=n(m[d]['gates']), hs=n(m[d]['hs']), cs=n(m[d]['cs']))


@pytest.mark.parametrize('case', PC.ENCODER, ids=lambda c: 'B%d-T%d-L%d' % c)
def test_encoder_forward_against_float64_at_every_edge(case):
    enc, w = encoder_module()
    seq, lens = PC.encoder_tokens(case.B, case.T, case.Lpad)
    assert max(lens) == case.T
    for train in (False, True):
        what = 'encoder B%d T%d L%d %s' % (case.B, case.T, case.Lpad, 'train' if train else 'eval')
        g, ran = encoder_fwd(enc, dev(seq), lens, True, train)
        assert ran == [PC.ENC_KERNEL], ran
        for k, v in g.items():
            assert v.untouched(whole=(k == 'xg')), 'guard rows of %s were written' % k      # (with the table nobody writes xg)
        out = {k: g[k].np() for k in ENC_KEYS}
        mask = drop_mask(train, case.B, case.T * H)
        r64 = model_tensors(PC.encoder_model(w, seq, lens, mask))
        r32 = model_tensors(PC.encoder_model(w, seq, lens, mask, torch.float32))
        PC.compare(what, out, r64, r32, ENC_KEYS, rows=ROWS)
        PC.check_ctx_beyond_lengths(out['ctx'], lens)
        PC.check_state_held(out['hs'], out['cs'], lens)
        assert not out['hs'][0].any() and not out['cs'][0].any()
        if train:
            assert np.array_equal(out['ctx'] == 0, r64['ctx'] == 0), 'the ctx dropout mask is not the mirror\'s'


def test_one_step_past_the_encoder_limit_falls_back_bit_for_bit():
    case = PC.ENCODER_FALLBACK
    enc, w = encoder_module()
    seq, lens = PC.encoder_tokens(case.B, case.T, case.Lpad)
    a, ran_a = encoder_fwd(enc, dev(seq), lens, True, False)
    b, ran_b = encoder_fwd(enc, dev(seq), lens, False, False)
    assert ran_a == [] and ran_b == []
    for k in ENC_KEYS:
        assert torch.equal(a[k].t, b[k].t), k
        assert a[k].untouched()


# ------------------------------------------------------------------- recurrence with an initial state
@pytest.mark.parametrize('case', PC.TEACHER, ids=lambda c: 'B%d-S%d-v%d-Tp%d' % c)
def test_teacher_recurrence_with_an_initial_state(case):
    """sf_speaker_teacher_fwd (enc_persist_kernel with h_init, seq_st = B, lengths = NULL; the head for all S B rows at
    once) against the teacher-mode float64 word loop."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import ptr, ws_args
    B, S, V, Tp = case
    spk = PC._spk(vocab=V, Tp=Tp, B=B, S=S)
    dec, dec_w = decoder_module(V, False)
    inp = PC.speaker_inputs(spk)
    ldv = PC.ldv(V)
    g = dict(hs=Guarded(S + 1, B, H), cs=Guarded(S + 1, B, H), words=Guarded(S + 1, B, dtype=torch.int64, fill=WORD_SENTINEL),
             ended=Guarded(B, dtype=torch.uint8, fill=ENDED_SENTINEL), step_scores=Guarded(S, B), nll_term=Guarded(S, B),
             live=Guarded(S, B), gates=Guarded(S, B, 4 * H), cat2=Guarded(S, B, 2 * H), t_text=Guarded(S, B, H),
             alpha=Guarded(S, B, Tp), h_tilde=Guarded(S, B, H), logit=Guarded(S, B, ldv))
    g['hs'].t[0] = dev(inp.h_init)
    g['cs'].t[0] = dev(inp.c_init)
    g['words'].t[0] = BOS
    g['ended'].t.zero_()
    BH = B * H
    addr = lambda k, off=0: g[k].full.data_ptr() + 4 * off                 # noqa: E731
    tp0 = _lib.SpkDecoderTape(None, addr('gates'), addr('cs', BH), addr('hs', BH), addr('cat2'), addr('t_text'), addr('alpha'),
                              addr('h_tilde'), addr('logit'))
    ins = [dev(a) for a in (inp.targets, inp.ctx, inp.mask)]
    w = dec._w_struct(table=True)
    with _lib.kernel_profile() as prof:
        rc = _lib.lib.sf_speaker_teacher_fwd(C.byref(w), B, E, H, Tp, V, S, PAD, EOS, ptr(ins[0]), g['hs'].ptr(), g['cs'].ptr(),
                                             ptr(ins[1]), ptr(ins[2]), g['words'].ptr(), g['ended'].ptr(), g['step_scores'].ptr(),
                                             g['nll_term'].ptr(), g['live'].ptr(), C.byref(tp0), None, 0,
                                             *ws_args(torch.device('cuda')))
        torch.cuda.synchronize()
    no_fault('sf_speaker_teacher_fwd %s' % (case,))
    assert rc == 0 and persistent_kernels(prof) == [PC.ENC_KERNEL], (rc, persistent_kernels(prof))
    for k, v in g.items():
        assert v.untouched(), 'guard rows of %s were written' % k
    words = g['words'].np()
    assert np.array_equal(words, PC.teacher_words(inp, B))
    logit = g['logit'].np()
    assert np.isnan(logit[..., V:]).all()
    out = dict(logits=logit[..., :V], alpha=g['alpha'].np(), h1=g['hs'].np()[1:], c1=g['cs'].np()[1:],
               step_scores=g['step_scores'].np(), nll_term=g['nll_term'].np(), live=g['live'].np(), ended=g['ended'].np())
    r64 = PC.word_loop(dec_w, inp, words)
    r32 = PC.word_loop(dec_w, inp, words, torch.float32)
    PC.compare('teacher recurrence B%d S%d v%d Tp%d' % case, out, r64, r32, PC.TENSORS, rows=ROWS)
    PC.check_exact_flags(out, r64, words)
    PC.check_alpha(out['alpha'], inp.mask)


# ----------------------------------------------------------------------------------- encoder backward
LSTM_GRADS = ('lstm.weight_ih_l0', 'lstm.weight_hh_l0', 'lstm.bias_ih_l0', 'lstm.bias_hh_l0')


def encoder_bwd(enc, g, lens, dctx, d_init, d_ct, train, persistent):
    """sf_encoder_lstm_bwd on the forward tape `g` (encoder_fwd's buffers): (dgates tape, weight gradients, persistent
    kernels that ran).  The gradients of `enc` are reset first."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.model import _encoder_structs
    from speaker_follower_amd.runtime import ptr, ws_args, dropout_arg
    B, T = len(lens), max(lens)
    for p in enc.parameters():
        p.grad = None
    enc.persistent = persistent
    try:
        dg = Guarded(T, B, 4 * H)
        tp = _lib.EncoderTape(g['emb'].full.data_ptr(), dg.full.data_ptr(), g['gates'].full.data_ptr(), g['hs'].full.data_ptr(),
                              g['cs'].full.data_ptr())
        ws, gs = _encoder_structs(enc), _encoder_structs(enc, grad=True)
        lens_dev = torch.tensor(lens, dtype=torch.int32, device='cuda')
        with _lib.kernel_profile() as prof:
            _lib.call('sf_encoder_lstm_bwd', C.byref(ws), C.byref(gs), B, T, E, H, ptr(lens_dev), g['h'].ptr(), ptr(dctx),
                      ptr(d_init), ptr(d_ct), C.byref(tp), dropout_arg(*(DROP if train else (0.0, 0))), SITE,
                      *ws_args(dctx.device))
            torch.cuda.synchronize()
    finally:
        enc.persistent = True
    no_fault('sf_encoder_lstm_bwd B=%d T=%d' % (B, T))
    return dg, {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}, persistent_kernels(prof)


def reference_grads(w, seq, lens, mask, up, dtype, bidir):
    """Autograd of torch_ref.encoder_lstm / encoder_bilstm in `dtype` under the loss sum(ctx dctx) + sum(h d_init) +
    sum(c d_ct): {parameter: gradient}; and the retained gradients of the model's pre-activation gates per direction."""
    tw = torch_ref.to_torch(w, requires_grad=True, frozen=('embedding.weight',), dtype=dtype)
    fn = torch_ref.encoder_bilstm if bidir else torch_ref.encoder_lstm
    dctx, d_init, d_ct = (torch.as_tensor(a).to(dtype) for a in up)
    dm = None if mask is None else torch.as_tensor(mask).to(dtype).reshape(dctx.shape)
    ctx, h, c = fn(tw, torch.as_tensor(seq), lens, drop_ctx=dm)
    ((ctx * dctx).sum() + (h * d_init).sum() + (c * d_ct).sum()).backward()
    grads = {k: p.grad.double().numpy() for k, p in tw.items() if p.grad is not None}
    m = PC.encoder_model(w, seq, lens, mask, dtype, grad=True)
    ((m['ctx'] * dctx).sum() + (m['decoder_init'] * d_init).sum() + (m['c_t'] * d_ct).sum()).backward()
    dg = {'dgates_' + d: torch.stack([p.grad for p in m[d]['pre']]).double().numpy() for d in ('f', 'r') if d in m}
    return grads, dg


@pytest.mark.parametrize('case', PC.ENCODER_BWD, ids=lambda c: 'B%d-T%d%s%s' % (c.B, c.T, '-train' if c.train else '',
                                                                                 '-bidir' if c.bidir else ''))
def test_encoder_backward_against_float64_autograd(case):
    from speaker_follower_amd import _lib, model
    from speaker_follower_amd.runtime import dropout_arg
    B, T, train, bidir = case
    enc, w = encoder_module(bidir)
    Hd, nd = (PC.H_BI, 2) if bidir else (H, 1)
    seq, lens = PC.encoder_tokens(B, T, T if bidir else max(T, 8))
    seq_dev = dev(seq)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device='cuda')
    rng = np.random.default_rng([B, T, 47])
    up = [rng.standard_normal(s).astype(np.float32) for s in ((B, T, nd * Hd), (B, nd * Hd), (B, nd * Hd))]
    dctx, d_init, d_ct = (dev(a) for a in up)
    drop = dropout_arg(*(DROP if train else (0.0, 0)))
    for p in enc.parameters():
        p.grad = None
    enc.persistent = True
    what = 'encoder backward B%d T%d%s%s' % (B, T, ' train' if train else '', ' bidir' if bidir else '')
    if bidir:
        tapes = [dict(emb=Guarded(T, B, E), xg=Guarded(T, B, 4 * Hd), gates=Guarded(T, B, 4 * Hd), hs=Guarded(T + 1, B, Hd),
                      cs=Guarded(T + 1, B, Hd)) for _ in range(2)]
        plain = [{k: v.t for k, v in tp.items()} for tp in tapes]
        ctx, dinit, c_t = Guarded(B, T, 2 * Hd), Guarded(B, 2 * Hd), Guarded(B, 2 * Hd)
        with _lib.kernel_profile() as prof:
            model.bi_encoder_fwd(enc, seq_dev, lens_dev, T, drop, SITE, True, plain, ctx.t, dinit.t, c_t.t)
            model.bi_encoder_bwd(enc, seq_dev, lens_dev, T, drop, SITE, True, plain, dinit.t, dctx, d_init, d_ct)
            torch.cuda.synchronize()
        no_fault(what)
        assert enc.last_path == enc.last_backward_path == 'persistent'
        assert set(persistent_kernels(prof)) == {PC.ENC_BI_KERNEL, PC.ENC_BWD_BI_KERNEL}, persistent_kernels(prof)
        for tp in tapes:
            for k, v in tp.items():
                assert v.untouched(), 'guard rows of %s were written' % k
        assert ctx.untouched() and dinit.untouched() and c_t.untouched()
        got_dg = {'dgates_f': tapes[0]['xg'].np(), 'dgates_r': tapes[1]['xg'].np()}
    else:
        g, ran = encoder_fwd(enc, seq_dev, lens, True, train)
        assert ran == [PC.ENC_KERNEL]
        dg, _, ran = encoder_bwd(enc, g, lens, dctx, d_init, d_ct, train, True)
        assert ran == [PC.ENC_BWD_KERNEL], ran
        assert dg.untouched()
        got_dg = {'dgates_f': dg.np()}
    hip = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    mask = drop_mask(train, B, T * nd * Hd)
    g64, dg64 = reference_grads(w, seq, lens, mask, up, torch.float64, bidir)
    g32, dg32 = reference_grads(w, seq, lens, mask, up, torch.float32, bidir)
    names = LSTM_GRADS + (tuple(k + '_reverse' for k in LSTM_GRADS) if bidir else ()) + ('encoder2decoder.weight', 'encoder2decoder.bias')
    assert set(names) <= set(hip) and set(names) <= set(g64), (sorted(hip), sorted(g64))
    for k in got_dg:
        assert np.isfinite(got_dg[k]).all(), k
    PC.compare(what, got_dg, dg64, dg32, sorted(got_dg), rows=ROWS)
    for k, v in got_dg.items():
        for b, n in enumerate(lens):
            assert not v[n:, b].any(), 'dgates of row %d are not zero behind its length' % b
    GC.compare_grads(hip, {k: g64[k] for k in names}, g32, what=what)


@pytest.mark.parametrize('persistent', [True, False], ids=['persistent', 'per_step'])
def test_dctx_beyond_a_length_reaches_nothing(persistent):
    """ctx beyond a row's length is the constant 0 (model.py:101): whatever dctx holds there -- training hands zeros, the
    text attention masks those positions -- must reach no state and no weight gradient.  The first run of
    test_encoder_backward_against_float64_autograd found all three forms of the backward step adding it to dh, which a dead
    step passes on to the row's last live one (dgates off by 0.4 .. 4 of their scale under a random dctx)."""
    enc, w = encoder_module()
    B, T = 9, 5
    seq, lens = PC.encoder_tokens(B, T, 8)
    rng = np.random.default_rng(53)
    dctx = rng.standard_normal((B, T, H)).astype(np.float32)
    clean = dctx.copy()
    for b, n in enumerate(lens):
        clean[b, n:] = 0
        dctx[b, n:] = np.float32('nan') if b % 2 else 1e30
    d_init, d_ct = (dev(rng.standard_normal((B, H)).astype(np.float32)) for _ in range(2))
    g, _ = encoder_fwd(enc, dev(seq), lens, True, True)
    dg_a, gr_a, ran = encoder_bwd(enc, g, lens, dev(clean), d_init, d_ct, True, persistent)
    assert ran == ([PC.ENC_BWD_KERNEL] if persistent else [])
    dg_b, gr_b, _ = encoder_bwd(enc, g, lens, dev(dctx), d_init, d_ct, True, persistent)
    assert torch.equal(dg_a.t, dg_b.t) and not torch.isnan(dg_b.t).any()
    assert sorted(gr_a) == sorted(gr_b) and len(gr_a) >= 6
    for k in gr_a:
        assert torch.equal(gr_a[k], gr_b[k]), k
