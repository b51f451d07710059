"""GPU: the speaker's `sample` draw (csrc/sf_sampling.h) in its three kernels, each alone, held to the float64 mirror
oracle.rng.speaker_sample on EVERY row (tests/speaker_sample_cases.py: the launches, the rule `check_draws`, the float32
models of the summation orders; tests/test_speaker_sample_cases_host.py proves those on the CPU):

    1  sf_speaker_glue_fwd, feedback 2    speaker_glue_kernel (vocab 37, 991, 1024) and speaker_glue_wide_sample_kernel
                                          (1025, 1086, 4096): 256 rows per launch over poisoned padding columns, the plain
                                          launch at two seeds and one launch per edge uniform (u1, u2 = 0, 1 - 2^-24, 0.5)
    2  sf_speaker_decode, feedback 2      spk_persist_kernel<sample> at the vocabularies of persist_cases.SAMPLE_VOCABS:
                                          decoder2action.weight = 0 and the constructed row in decoder2action.bias, so every
                                          (step, row) logit IS the bias and the 36 draws of a launch differ in their
                                          uniforms alone; the edge uniform falls at step 1, row 4.  B 9, S 4: the smallest
                                          shape of persist_cases.SPEAKER that has a step behind step 0.
    3  the kernels together               up to 1024 words the glue draws the persistent loop's word on every CLEAR
                                          (step, row) of the same logits and uniforms

The rule: a row whose margin exceeds its floor (1e-5 up to 1024 words, 1e-5 * slots / 32 above) is CLEAR and takes the
mirror's word; an unclear row takes one of the mirror's words at (u1, u2) and the four corners u (1 +- 1e-5); no row is
skipped; every word lies in [0, vocab), has a finite logit within 104 of its slot's maximum (a float32 weight above 0), and
its slot a finite maximum; the u = 0.5 rows, exact in float32, take the mirror's word.  score = log p(word) follows
tests/grad_compare.py (K = 4, floor 1e-5) against the float64 log-softmax, and is bit for bit the score of a teacher launch
on the drawn words, as is `ended`; nll_term and live are bit for bit those of a teacher launch on the same targets.
Every case keeps a clear share of at least 0.99 on the mirror alone (a condition on the inputs, asserted in the host module;
for the word loop over the launches of one vocabulary together: speaker_sample_cases._persist_all says why).

WHAT THE FIRST RUN FOUND, on the kernels as they were (62 of the 174 launches failed), all fixed with this module:
  a  level 2 fell back to the slot's last column, min(32 s + 31, V - 1), when no column passed u2 z_s.  At u2 = 1 - 2^-24
     on a slot whose last 5 columns are dead the device drew a word of float32 probability exactly 0:
       speaker_glue_kernel        vocab 37: word 31 (mirror 26); 991: 959 (954); 1024: 991 (986) -- with the tail 111 ..
                                  123 below the slot's maximum, and again with the tail at -inf (score -inf)
       the wide kernel            1025: 1023 (1018) and 4096: 4063 (4058) on the underflowed tail; 1086: 1055 (1050) and
                                  4096: 4063 on the -inf tail.  At 1025 / -inf and 1086 / underflow a column passed on the
                                  device although the float32 order model predicted none (it predicts, it does not define)
       spk_persist_kernel<sample> all five vocabularies on the underflowed tail: words 31, 31, 447, 927, 991 (mirror 26, 26,
                                  442, 922, 986); on the -inf tail a column passed in the word loop (the mirror's word), while
                                  the glue on the same row and uniforms took the fallback
     Now the fallback is the slot's last column with e > 0, in all three kernels and in the mirror.
  b  speaker_sample_row formed expf(l - m_s) with m_s = -inf for a slot of 32 banned words: NaN in z_s, in the slot's weight,
     through the shuffle scan in every later lane and in Z, so `cdf > u1 Z` held nowhere and EVERY row with an empty slot drew
     from the arg max's slot: 18 .. 23 clear rows of the 256 differed from the mirror in each of the 16 launches at 991 and
     1024 words that do not stop at (a) first (none at 37: with two slots the one that is left is the arg max's).  Now
     wexp, as in the wide kernel.
  c  not predicted: the word loop formed its slot statistics the same way (phase G, every feedback): an empty slot
     published z_s = NaN, wexp(m_s) * NaN stayed NaN in Z, and step_scores and nll_term were NaN at every (step, row) of
     every launch whose bias bans a whole slot (6 launches at 33 words, 7 each at 480, 935, 1024; the words came from the arg
     max's slot).  Now wexp there too -- the same bits wherever the slot's maximum is finite, which the bit-for-bit tests of
     tests/test_gpu_persistent_edges.py hold; test_word_loop_statistics_survive_an_empty_slot pins teacher and argmax.
  -inf bias columns pass through the word loop: the logits tape holds them, nothing else is non-finite.

Measured on an MI355X after the fixes (`-s` prints every figure):
    clear share      glue: 1.0000 in 22 launches, 255 / 256 in 33, 254 / 256 in 11 (the edge row unclear by design in 30);
                     word loop: 1.0000 in 108 launches, 35 / 36 in 26; per vocabulary 0.9921 .. 0.9962
    unclear rows     81 in all; 77 took the mirror's word at (u1, u2).  The other 4 are u1 = 1 - 2^-24 rows on which no
                     slot passed and the word came from the arg max's slot, as the kernel's own order model predicted:
                     speaker_glue_kernel at 991 words (word 29, the mirror's 907 lies in the last slot that carries weight),
                     the wide kernel at 1025 (4 for 975), the word loop at 480 (21 for 394) and at 935 (20 for 874).  At
                     1024 (glue and loop), 1086 and 4096 a slot passed on the device although the model predicted none.
                     Both u = 0.5 rows of every vocabulary took the second of the two equal weights.
    score            rows near 0: worst e / e32 = 3.5 in the sampled launches (word loop, 935 words: 1.3e-06 / 3.9e-07,
                     bound 1.0e-05) and 4.4 in the argmax launch over two empty slots (3.9e-07 / 8.8e-08, the floor 1e-05
                     decides); glue 1.7 (1.8e-06 / 1.0e-06); rows shifted +-80: 1.16 (4.6e-06 / 4.0e-06, bound 1.6e-05).
                     Nothing above 0.3 of its bound.  Bit-equal to the teacher launch on the drawn words everywhere.
    together         up to 1024 words 789 .. 1003 clear draws per vocabulary, the same word in the glue and the word loop
    wall time        5.4 s for the module's 69 tests, 0.48 s in the slowest (4096 words, u1 = 1 - 2^-24: the row is drawn
                     until the order model misses)

Sensitivity: one value-only error planted per scratch build (never committed: every word stays inside the row), this
module run on each.  Counts are failing tests of the module's 69: a glue test is one launch; a word loop test covers the
22 .. 28 launches of one vocabulary, stops at its first failure, and also fails when the glue half of section 3 does.
    speaker_glue_kernel (tests at 37, 991, 1024 words) and the wide kernel (1025, 1086, 4096), planted together:
      `>=` for `>` at level 2            3 + 3: every u2 = 0.5 launch drew the first column of the pair
      `>=` for `>` at level 1            3 + 3: every u1 = 0.5 launch drew word 5, the first slot of the pair
      `e > 0` dropped at level 2         0 + 0: see below
      `ps > 0` dropped at level 1        1 + 1: the u1 = 1 - 2^-24 launches at 991 (word 990) and 1025 (word 1023), words
                                         of a slot with no finite column
      fallback column back at 32 s + 31  6 + 4: the launches of finding (a)
      expf for wexp (glue) / `carry`     20 + 30: every launch at 991 and 1024 words; every launch of the wide kernel
      not added (wide)
      u1 and u2 swapped                  30 + 30: every launch
      (each of these also fails 3 .. 5 of the word loop tests through the glue half of section 3)
    spk_persist_kernel<sample>, planted alone (5 word loop tests, 2 statistics tests; no glue test fails):
      `>=` for `>` in row16_pick32       5: level 2 at 32 words (u2 = 0.5: word 7 for 23), level 1 at 33 .. 1024
                                         (u1 = 0.5: word 5 for the last slot's)
      weight guards dropped there        4: level 2 at 32, 33 and 1024 words (u2 = 1 - 2^-24: words 28, 28, 988 of the dead
                                         tail), level 1 at 480 (u1 = 1 - 2^-24: a draw from an empty slot, score -inf)
      fallback column back at 32 s + 31  4
      expf for wexp in the statistics    4 + the 2 statistics tests
      u1 and u2 swapped                  5
  The one plant without a failure changes no word: in the two glue kernels the level-2 prefix is a running sum in column
  order (lane 2 s + 1 goes on from lane 2 s's total), so it is level over zero weights and a zero-weight column can pass
  only if the column before it did; the guard is redundant there and no input can show its absence.  In the word loop
  every lane's prefix is rounded in an order of its own, and there the guard is what keeps a dead column out.  The
  level-1 guards are held by the u1 = 1 - 2^-24 rows alone, at the vocabularies where the device does take the fallback.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import persist_cases as PC                                 # noqa: E402
from tests import speaker_sample_cases as SC                          # noqa: E402
from tests import test_gpu_persistent_edges as PE                     # noqa: E402  (decode, Guarded, no_fault)
from tests import test_gpu_speaker_wide_sample as WS                  # noqa: E402  (_glue: poisoned padding columns)

F32 = np.float32
PAD, EOS = WS.PAD, WS.EOS
GLUE_KERNEL = {True: 'speaker_glue_wide_sample_kernel', False: 'speaker_glue_kernel'}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def glue(logit, target, feedback, seed, stream, row0):
    """WS._glue under the kernel profile -> (w, score, ended, nll, live, names of the glue kernels that ran)."""
    from speaker_follower_amd import _lib
    with _lib.kernel_profile() as prof:
        out = WS._glue(logit, target, feedback, seed, stream, row0)
    return out + (sorted(k for k in prof.rows if k.startswith('speaker_glue')),)


def report(what, res, scores=()):
    print('[sample] %-34s clear %.4f  unclear rows %s' % (what, res['share'], res['unclear']))


# ---- 1. the per-step glue -----------------------------------------------------------------------------------------------
def check_glue_launch(vocab, special, seed, row0_shift=0, stream_shift=0):
    case = SC.speaker_sample_case(vocab, special, seed)
    ex = SC.case_expectation(vocab, special, seed, row0_shift, stream_shift)
    what = 'glue v%d %s seed %d%s' % (vocab, special or 'plain', seed, ' moved' if row0_shift or stream_shift else '')
    x = case['logit']
    dl = torch.from_numpy(x).cuda()
    target = torch.from_numpy(case['target']).cuda()
    at = (case['seed'], case['stream'] + stream_shift, case['row0'] + row0_shift)
    w, score, ended, nll, live, ran = glue(dl, target, 2, *at)
    assert ran == [GLUE_KERNEL[vocab > 1024]], ran
    if special and not row0_shift and not stream_shift:
        i = case['at']
        print('[sample] %s: row %d drew %d (mirror %d, allowed %s; logit %s, slot max %s)' % (
            what, i, w[i], ex['w'][i], sorted(ex['allowed'][i]), x[i, min(max(int(w[i]), 0), vocab - 1)],
            x[i, 32 * (int(w[i]) // 32):32 * (int(w[i]) // 32) + 32].max()))
    res = SC.check_draws(what, w, x, ex)
    scores = SC.check_scores(what, score, x, w, PAD)
    # the loss terms do not depend on the feedback: those of a teacher launch on the same targets, bit for bit
    _, _, _, nll0, live0, ran0 = glue(dl, target, 0, *at)
    assert ran0 == ['speaker_glue_kernel']
    assert np.array_equal(bits(nll), bits(nll0)) and np.array_equal(bits(live), bits(live0)), what
    assert np.isfinite(nll).all()
    # a teacher launch ON THE DRAWN WORDS: the same score and the same flags, bit for bit
    _, score1, ended1, _, _, _ = glue(dl, torch.from_numpy(w).cuda(), 0, *at)
    assert np.array_equal(bits(score), bits(score1)), what
    assert np.array_equal(ended, ended1) and np.array_equal(ended, (w == EOS).astype(np.uint8)), what
    report(what, res, scores)
    return w, ex


@pytest.mark.parametrize('vocab,special,seed', SC.GLUE_CASES, ids=lambda v: str(v))
def test_glue_draw_equals_the_mirror_on_every_row(vocab, special, seed):
    assert SC.margin_floor(vocab) == (WS._margin_floor(vocab) if vocab > 1024 else 1e-5)
    w, ex = check_glue_launch(vocab, special, seed)
    if special is None:
        assert len(np.unique(w)) > 20                                   # it is not the arg max in disguise


@pytest.mark.parametrize('vocab', [991, 1086])
def test_glue_draw_is_addressed_by_global_row_and_stream(vocab):
    """The same logits at another row0 and at a second stream: the uniforms are those of the GLOBAL rows at that stream."""
    w0, _ = check_glue_launch(vocab, None, 0)
    w1, _ = check_glue_launch(vocab, None, 0, row0_shift=7777)
    w2, _ = check_glue_launch(vocab, None, 0, stream_shift=5)
    assert (w0 != w1).mean() > 0.5 and (w0 != w2).mean() > 0.5 and (w1 != w2).mean() > 0.5


# ---- 2. / 3. the persistent word loop, and the kernels together --------------------------------------------------------------
def zero_weight_decoder(vocab):
    """A SpeakerDecoderLSTM whose decoder2action.weight is zero: the logits of every (step, row) are its bias."""
    from speaker_follower_amd import model
    w = dict(PC.speaker_decoder_weights(vocab, False))
    w['decoder2action.weight'] = np.zeros_like(w['decoder2action.weight'])
    dec = model.SpeakerDecoderLSTM(vocab, PE.E, PE.H, 0.5, glove=w['embedding.weight'])
    dec.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return dec.cuda().eval()


def check_loop_launch(vocab, index, dec, case, inp0):
    """One launch of the word loop on one constructed row (section 2), then S launches of the per-step glue on the same
    logits and uniforms (section 3) -> (check_draws' result, the mirror's side, clear draws equal in both kernels)."""
    from speaker_follower_amd import _lib
    B, S = case.B, case.S
    name, row, stream, row0, info = SC.persist_rows(vocab)[index]
    what = 'loop v%d %s' % (vocab, name)
    ex = SC.persist_expectation(vocab, index)
    dec.decoder2action.bias.data.copy_(torch.from_numpy(row))
    fin = np.flatnonzero(np.isfinite(row))
    inp = inp0._replace(targets=np.full((S, B), fin[len(fin) // 2], np.int64))          # a finite NLL at every step
    rc, out, g, ran = PE.decode(dec, case, inp, 'sample', sample=_lib.Sample(SC.SEED, stream, row0, None))
    assert rc == 0 and ran == [PC.SPK_SAMPLE_KERNEL], (what, rc, ran)
    PE.guards_untouched(g)
    assert np.isnan(out['logits_pad']).all(), what
    words = out['words']
    assert (words[0] == PC.BOS).all()
    w = words[1:].reshape(-1)
    logit = np.tile(row, (S * B, 1))
    if info is not None:
        i = SC.P_T * B + SC.P_ROW
        print('[sample] %s: step %d row %d drew %d (mirror %d, allowed %s; logit %s)' % (
            what, SC.P_T, SC.P_ROW, w[i], ex['w'][i], sorted(ex['allowed'][i]), row[min(max(int(w[i]), 0), vocab - 1)]))
    # the logits tape IS the bias, bit for bit: -inf columns pass through, nothing else is non-finite
    assert np.array_equal(bits(out['logits']), np.broadcast_to(bits(row), (S, B, vocab))), what
    for k in ('step_scores', 'nll_term', 'live', 'alpha', 'h1', 'c1'):
        assert np.isfinite(out[k]).all(), '%s: %s holds non-finite values' % (what, k)
    res = SC.check_draws(what, w, logit, ex)
    scores = SC.check_scores(what, out['step_scores'].reshape(-1), logit, w, PAD)
    assert np.array_equal(out['ended'], (words[1:] == EOS).any(0).astype(np.uint8)), what
    report(what, res, scores)
    together = 0
    dl = torch.from_numpy(logit[:B]).cuda()
    tg = torch.from_numpy(inp.targets[0]).cuda()
    for t in range(S):
        wg, _, _, _, _, ran_g = glue(dl, tg, 2, SC.SEED, stream + t, row0)
        assert ran_g == ['speaker_glue_kernel']
        sel = slice(t * B, (t + 1) * B)
        SC.check_draws(what + ' (glue, step %d)' % t, wg, logit[:B], {k: v[sel] for k, v in ex.items()})
        cl = ex['clear'][sel]
        assert np.array_equal(wg[cl], w[sel][cl]), '%s step %d: the glue and the word loop draw different words' % (what, t)
        together += int(cl.sum())
    return res, ex, together


@pytest.mark.parametrize('vocab', SC.PERSIST_VOCABS)
def test_word_loop_draw_equals_the_mirror_on_every_step_and_row(vocab):
    assert SC.PERSIST_VOCABS == PC.SAMPLE_VOCABS and (SC.P_B, SC.P_S) == (PC.SPK_DEFAULT['B'], PC.SPK_DEFAULT['S'])
    case = PC._spk(vocab=vocab)
    dec = zero_weight_decoder(vocab)
    inp0 = PC.speaker_inputs(case)
    clear, unclear, together = [], [], 0
    for index in range(len(SC.persist_rows(vocab))):
        res, ex, n = check_loop_launch(vocab, index, dec, case, inp0)
        clear.append(ex['clear'])
        unclear += res['unclear']
        together += n
    share = float(np.concatenate(clear).mean())
    print('[sample] loop v%d: %d launches, clear share %.4f, %d unclear draws; %d clear draws equal in glue and loop' % (
        vocab, len(clear), share, len(unclear), together))
    assert share >= 0.99


@pytest.mark.parametrize('feedback', ['teacher', 'argmax'])
def test_word_loop_statistics_survive_an_empty_slot(feedback):
    """What section 2 found beside the draw: a slot of 32 banned words (bias -inf) published z_s = NaN, and the NaN
    reached the log-sum-exp of every row at EVERY feedback.  With two empty slots the scores and the NLL are finite and
    equal the float64 log-softmax of the bias row under the rule."""
    vocab = 935
    case = PC._spk(vocab=vocab)
    B, S = case.B, case.S
    dec = zero_weight_decoder(vocab)
    row = next(r for n, r, _, _, _ in SC.persist_rows(vocab) if n == 'empty2')
    assert sum(not np.isfinite(row[c:c + 32]).any() for c in range(0, vocab, 32)) == 2
    dec.decoder2action.bias.data.copy_(torch.from_numpy(row))
    fin = np.flatnonzero(np.isfinite(row))
    targets = np.tile(fin[np.arange(B) * 7 % len(fin)], (S, 1)).astype(np.int64)
    targets[:, B - 1] = PAD
    rc, out, g, ran = PE.decode(dec, case, PC.speaker_inputs(case)._replace(targets=targets), feedback)
    assert rc == 0 and ran == [PC.SPK_KERNEL]
    PE.guards_untouched(g)
    assert np.array_equal(bits(out['logits']), np.broadcast_to(bits(row), (S, B, vocab)))
    w = out['words'][1:]
    assert np.array_equal(w, targets if feedback == 'teacher' else np.full((S, B), int(np.argmax(row))))
    logit = np.tile(row, (S * B, 1))
    SC.check_scores('loop v935 empty2 %s' % feedback, out['step_scores'].reshape(-1), logit, w.reshape(-1), PAD)
    nll = SC.CM.lse(logit, np.float64) - logit.astype(np.float64)[np.arange(S * B), targets.reshape(-1)]
    nll32 = SC.CM.lse(logit, F32) - logit[np.arange(S * B), targets.reshape(-1)]
    live = targets.reshape(-1) != PAD
    SC.CM.check_values('loop v935 empty2 %s nll' % feedback, out['nll_term'].reshape(-1), np.where(live, nll, 0), np.where(live, nll32, 0))
    assert np.array_equal(out['live'].reshape(-1), live.astype(F32))
