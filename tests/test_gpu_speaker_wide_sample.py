"""GPU: `sample` feedback of the speaker (speaker.py:170-174) over vocabularies of more than 1 024 words -- the
reference's trainval vocabulary has 1 086 -- by speaker_glue_wide_sample_kernel (csrc/sf_pointwise.hip): the two-level
draw of csrc/sf_sampling.h over ceil(vocab / 32) slots in panels of 1 024 columns.  Checked draw by draw against the
float64 mirror (oracle/rng.py::speaker_sample, any width), against softmax by chi-square, and through every layer
that carries the opt-in switch `wide_sample`: SpeakerEngine (score / capture), SpeakerSweep, Seq2SeqSpeaker."""
import copy
import ctypes as C
import dataclasses
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rng as orng                                        # noqa: E402  (checker only)
from speaker_follower_amd import synth                                # noqa: E402

PAD, EOS = 0, 2
VOCAB = 1086                                                          # tasks/R2R/data/trainval_vocab.txt + 4 base tokens


def _glue(logit, target, feedback, seed, stream, row0=0):
    """sf_speaker_glue_fwd on [B,vocab] logits laid out with ldv = vocab rounded up to 4, plus 4: the columns
    [vocab, ldv) hold NaN and 1e30 alternately -- a kernel that reads one of them shows it in every output."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import ptr, stream as cur
    B, V = logit.shape
    ldv = ((V + 3) & ~3) + 4
    lg = torch.empty(B, ldv, device='cuda')
    lg[:, V::2] = float('nan')
    lg[:, V + 1::2] = 1e30
    lg[:, :V] = logit
    w = torch.empty(B, dtype=torch.int64, device='cuda')
    score, nll, live = (torch.empty(B, device='cuda') for _ in range(3))
    ended = torch.zeros(B, dtype=torch.uint8, device='cuda')
    smp = C.byref(_lib.Sample(seed, stream, row0)) if feedback == 2 else None
    _lib.call('sf_speaker_glue_fwd', B, V, ldv, ptr(lg), ptr(target), feedback, PAD, EOS, ptr(ended), ptr(w), ptr(score),
              ptr(nll), ptr(live), smp, cur())
    torch.cuda.synchronize()
    return w.cpu().numpy(), score.cpu().numpy(), ended.cpu().numpy(), nll.cpu().numpy(), live.cpu().numpy()


def _chi2(counts, p, n):
    from scipy import stats
    keep = p * n >= 5
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(p[keep] * n, p[~keep].sum() * n)
    if exp[-1] < 5:
        obs[-2] += obs[-1]
        exp[-2] += exp[-1]
        obs, exp = obs[:-1], exp[:-1]
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    return chi2, float(stats.chi2.sf(chi2, len(obs) - 1))


def _logp(logit):
    """float64 log-softmax along the last axis (-inf columns allowed)."""
    l64 = logit.astype(np.float64)
    mx = l64.max(-1, keepdims=True)
    return l64 - mx - np.log(np.exp(l64 - mx).sum(-1, keepdims=True))


def _margin_floor(vocab):
    """The existing tests skip a draw whose margin is <= 1e-5 at 32 slots; an fp32 prefix sum's error grows linearly
    with the number of slots it runs over."""
    return 1e-5 * ((vocab + 31) // 32) / 32


# ---- 1. the kernel alone, draw by draw ------------------------------------------------------------------------------
@pytest.mark.parametrize('vocab', [1025, 1056, 1086, 2048, 2049, 4095, 4096])
def test_wide_glue_sample_equals_the_mirror_draw_by_draw(vocab):
    g = np.random.default_rng(vocab)
    B = 512
    ns = (vocab + 31) // 32
    logit = (g.standard_normal((B, vocab)) * g.choice([0.3, 1.5, 4.0], size=(B, 1))).astype(np.float32)
    target = torch.from_numpy(g.integers(0, vocab, B)).cuda()
    # every 5th row: 40 scattered columns at -inf, none the first column of a slot, none in the (ragged) last slot
    free = np.array([c for c in range(32 * (ns - 1)) if c % 32])
    for b in range(0, B, 5):
        logit[b, g.choice(free, 40, replace=False)] = -np.inf
    logit[3::16, 32 * (ns - 1):] += 12.0                               # rows that draw from the last slot
    seed, stream, row0 = 0xC0FFEE, 17, 1000
    dl = torch.from_numpy(logit).cuda()
    w, score, ended, nll, live = _glue(dl, target, 2, seed, stream, row0)
    u1, u2 = orng.sample_uniforms(seed, stream, row0 + np.arange(B))
    with np.errstate(divide='ignore', invalid='ignore'):
        want = [orng.speaker_sample(logit[b], u1[b], u2[b]) for b in range(B)]
    clear = np.array([m > _margin_floor(vocab) for _, m in want])
    print('vocab %d: kept %.4f of the draws' % (vocab, clear.mean()))
    assert clear.mean() >= 0.98
    ww = np.array([x for x, _ in want])
    # the inputs exercise what they are meant to: the last slot, and the carry across panels
    print('vocab %d: last slot %.4f, at or beyond column 1024 %.4f' % (vocab, (ww >= 32 * (ns - 1)).mean(), (ww >= 1024).mean()))
    assert (ww >= 32 * (ns - 1)).mean() >= 0.04
    # (about half from 2 048 words up.  These are shares of the float64 MIRROR's words on the fixed inputs, nothing the
    # kernel computes: 0.496 at 2 048, 0.482 at 2 049, 0.760 at 4 095, 0.744 at 4 096 -- the expectation at 2 048 is
    # 1/16 + 15/16 * 1/2 = 0.53 with a binomial deviation of 0.022 over 512 rows)
    if vocab >= 2048:
        assert (ww >= 1024).mean() >= 0.48
    assert (w >= 0).all() and (w < vocab).all()
    assert np.isfinite(logit[np.arange(B), w]).all()
    assert np.array_equal(w[clear], ww[clear]), np.flatnonzero(clear & (w != ww))
    want_score = np.where(w != PAD, _logp(logit)[np.arange(B), w], 0.0)
    np.testing.assert_allclose(score, want_score, rtol=1e-4, atol=1e-4)            # speaker.py:179-180
    assert np.array_equal(ended, (w == EOS).astype(np.uint8))                     # :190-191
    # the loss terms do not depend on the feedback: bit for bit those of a teacher-forced launch
    _, _, _, nll0, live0 = _glue(dl, target, 0, seed, stream, row0)
    assert np.array_equal(nll.view(np.uint32), nll0.view(np.uint32))
    assert np.array_equal(live.view(np.uint32), live0.view(np.uint32))


# ---- 2. / 3. the distribution ---------------------------------------------------------------------------------------
def _follows_softmax(row, N, seed, stream):
    vocab = len(row)
    logit = torch.from_numpy(np.tile(row, (N, 1))).cuda()
    target = torch.zeros(N, dtype=torch.int64, device='cuda')
    w = _glue(logit, target, 2, seed, stream)[0]
    assert (w >= 0).all() and (w < vocab).all()
    assert np.isfinite(row[w]).all()                                   # no masked word is ever drawn
    p = np.exp(row.astype(np.float64) - row.max())
    p /= p.sum()
    chi2, pval = _chi2(np.bincount(w, minlength=vocab).astype(np.float64), p, N)
    print('chi2 %.1f, p %.4g' % (chi2, pval))
    assert pval > 1e-4, (chi2, pval)


def test_wide_glue_sample_never_draws_from_masked_slots():
    """Slots that are -inf throughout have weight 0 (wexp): the prefix walks over them, also over a masked LAST slot
    (oracle/rng.py gives NaN for such a slot, so the check is the distribution itself)."""
    g = np.random.default_rng(5)
    row = (g.standard_normal(VOCAB) * 1.5).astype(np.float32)
    row[32 * 3:32 * 21] = -np.inf                                      # slots 3 .. 20
    row[32 * 33:] = -np.inf                                            # the ragged last slot
    _follows_softmax(row, 20000, 99, 3)


@pytest.mark.parametrize('temp', [0.5, 2.5])
def test_wide_glue_sample_follows_softmax(temp):
    g = np.random.default_rng(5)
    row = (g.standard_normal(VOCAB) * temp).astype(np.float32)
    _follows_softmax(row, 20000, 99, 3)


# ---- 4. - 6. the engine, its graph, the sweep and the agent -----------------------------------------------------------
B_ENG, S_ENG, NVP = 12, 14, 48


@pytest.fixture(scope='module')
def wide():
    """The set-up of test_gpu_speaker.py::test_vocabulary_above_1024_runs_on_the_per_step_kernels."""
    from speaker_follower_amd import model, features
    d = dataclasses.replace(synth.FULL, vocab=VOCAB)
    senc_w, sdec_w = synth.speaker_weights_peaky(31, d)
    enc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    dec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    enc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    enc.cuda().eval()
    dec.cuda().eval()
    sb = synth.speaker_batch(seed=9, batch=B_ENG, n_viewpoints=NVP, min_path=3, max_path=5, min_len=4, max_len=S_ENG - 2,
                             dims=d)
    store = features.FeatureStore(synth.feature_table(7, NVP))
    return enc, dec, store, sb, d


def _engine(wide, **kw):
    from speaker_follower_amd import speaker
    enc, dec, store = wide[:3]
    eng = speaker.SpeakerEngine(enc, dec, store)
    for k, v in kw.items():
        setattr(eng, k, v)
    return eng


def _check_sampled_pass(wide, train):
    from speaker_follower_amd import speaker
    enc, dec, store, sb, _ = wide
    B, S = B_ENG, S_ENG
    batch = speaker.DeviceSpeakerBatch.from_synth(sb, row0=300)
    eng = _engine(wide, wide_sample=True, dropout_seed=0x1234)
    with torch.set_grad_enabled(train):
        st = eng.score(batch, S, 'sample', train=train)
    torch.cuda.synchronize()
    assert st.persistent is False and not st.teacher_path             # sf_speaker_words_fwd, as a 1 086-word argmax pass
    words = st.words.cpu().numpy()                                    # [S+1,B]
    logits = st.logits.detach().cpu().numpy()                         # [S,B,vocab]
    assert logits.shape[-1] == VOCAB and np.isfinite(logits).all()
    seed = (0x1234 ^ 0x3C6EF372) & 0xFFFFFFFF
    n_clear = n_all = 0
    for t in range(S):
        u1, u2 = orng.sample_uniforms(seed, st.site0 + t, 300 + np.arange(B))
        for b in range(B):
            w, margin = orng.speaker_sample(logits[t, b], u1[b], u2[b])
            n_all += 1
            if margin > _margin_floor(VOCAB):
                n_clear += 1
                assert words[t + 1, b] == w, (t, b, words[t + 1, b], w, margin)
    assert n_clear >= 0.98 * n_all
    assert ((words[1:] >= 0) & (words[1:] < VOCAB)).all()
    assert len(np.unique(words[1:])) > 5                              # it is not the arg max in disguise
    # scores = log p(sampled word)
    pick = np.take_along_axis(_logp(logits), words[1:, :, None], axis=2)[:, :, 0]
    want = np.where(words[1:] != PAD, pick, 0.0)
    np.testing.assert_allclose(st.step_scores.cpu().numpy(), want, rtol=1e-4, atol=2e-4)
    # the word fed back is the sampled one: teacher-forcing the sampled words (same dropout sites) gives the same logits
    b2 = copy.copy(batch)
    b2.instr_seq = torch.from_numpy(np.ascontiguousarray(words[1:].T)).cuda()
    ref = _engine(wide, persistent=False, dropout_seed=0x1234)
    ref.site_next = st.site0
    with torch.set_grad_enabled(train):
        rt = ref.score(b2, S, 'teacher', train=train)
    assert not rt.persistent
    la = rt.logits.detach().cpu().numpy()
    assert float(np.abs(la - logits).max()) <= 2e-4 * max(1.0, float(np.abs(la).max()))
    # sharding invariance: the second half of the rows alone, row0 shifted, draws the same words
    half = B // 2
    sub = type(sb)(**{k: (v[half:] if k in ('instr', 'path_len') else v[:, half:]) for k, v in sb.__dict__.items()})
    e2 = _engine(wide, wide_sample=True, dropout_seed=0x1234)
    with torch.set_grad_enabled(train):
        sh = e2.score(speaker.DeviceSpeakerBatch.from_synth(sub, row0=300 + half), S, 'sample', train=train)
    assert sh.site0 == st.site0
    assert (sh.words.cpu().numpy() == words[:, half:]).mean() > 0.97  # (a draw at a CDF boundary may flip and then diverge)


def test_engine_samples_at_1086_words_when_asked_to(wide):
    from speaker_follower_amd import speaker
    _check_sampled_pass(wide, train=False)
    # ... and only then: the default says so before anything is launched
    eng = _engine(wide)
    sites = eng.site_next
    batch = speaker.DeviceSpeakerBatch.from_synth(wide[3])
    for call in (eng.score, eng.run):
        with pytest.raises(NotImplementedError, match='wide_sample'):
            with torch.no_grad():
                call(batch, S_ENG, 'sample', train=False)
    with pytest.raises(NotImplementedError, match='wide_sample'):
        eng.capture(batch, S_ENG, 'sample')
    assert eng.site_next == sites


def test_engine_samples_at_1086_words_in_a_training_pass(wide):
    """One pass with dropout on (train=True), gradients enabled as in Seq2SeqSpeaker.train."""
    _check_sampled_pass(wide, train=True)


def test_captured_wide_sample_pass_draws_anew_on_every_replay(wide):
    """The pattern of tests/test_gpu_training_graph.py: the graph reads its sampling site from a device word."""
    from speaker_follower_amd import speaker
    batch = speaker.DeviceSpeakerBatch.from_synth(wide[3])
    eng = _engine(wide, wide_sample=True, dropout_seed=99)
    replay, st = eng.capture(batch, S_ENG, 'sample')
    assert st.persistent is False
    words, sites = [], []
    for _ in range(2):
        replay()
        torch.cuda.synchronize()
        words.append(st.words.cpu().numpy().copy())
        sites.append(st.site0)
    assert not np.array_equal(words[0], words[1])
    ref = _engine(wide, wide_sample=True, dropout_seed=99)
    for w, site in zip(words, sites):
        ref.site_next = site
        with torch.no_grad():
            e = ref.score(batch, S_ENG, 'sample', train=False)
        assert np.array_equal(e.words.cpu().numpy(), w)


def test_sweep_with_wide_sample_equals_the_engine(wide):
    from speaker_follower_amd import speaker
    enc, dec, store, _, d = wide
    sbs = [synth.speaker_batch(seed=100 + i, batch=B_ENG, n_viewpoints=NVP, min_path=4, max_path=4, min_len=4,
                               max_len=S_ENG - 2, dims=d) for i in range(3)]
    with pytest.raises(NotImplementedError, match='wide_sample'):
        speaker.SpeakerSweep(enc, dec, store, B_ENG, S_ENG, feedback='sample')
    sweep = speaker.SpeakerSweep(enc, dec, store, B_ENG, S_ENG, feedback='sample', wide_sample=True)
    out = sweep.run(sbs)
    assert sweep.fallbacks == 0 and len(sweep.graphs) == 1            # one path-step count: one graph, replayed 3 times
    (_, st, _, _), = sweep.graphs.values()
    assert st.persistent is False
    # the graph's engine numbers its replays' sampling sites in steps of site_stride; st.site0 is the last one's
    ref = _engine(wide, wide_sample=True, dropout_seed=torch.initial_seed() & 0xFFFFFFFF)
    for i, sb in enumerate(sbs):
        ref.site_next = st.site0 - (len(sbs) - 1 - i) * st.site_stride
        with torch.no_grad():
            e = ref.score(speaker.DeviceSpeakerBatch.from_synth(sb), S_ENG, 'sample', train=False)
        assert np.array_equal(out[i].astype(np.int64), e.words[1:].cpu().numpy()), i
    assert not np.array_equal(out[0], out[1])


def test_agent_samples_sentences_at_1086_words_when_asked_to(wide):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import search_world as W
    from speaker_follower_amd import agents, features
    enc, dec = wide[:2]
    rng_state = random.getstate()       # (the env reshuffles with the global generator when an epoch wraps)
    try:
        env, table = W.build_world(dense=False, n_items=24, batch=12, item_seed=5)
        spk = agents.Seq2SeqSpeaker(env, '/tmp/sf_spk_wide_sample.json', enc, dec, W.INSTRUCTION_LEN,
                                    max_episode_len=W.EPISODE_LEN)
        spk.store = features.FeatureStore(table)
        with pytest.raises(NotImplementedError, match='wide_sample'):
            spk.test(feedback='sample')
        spk.wide_sample = True
        res = spk.test(feedback='sample')
        assert spk._engine.wide_sample is True
        assert len(res) == 24
        ids = set()
        for r in res.values():
            wi = r['word_indices']
            assert 1 <= len(wi) <= W.INSTRUCTION_LEN and all(0 <= x < VOCAB for x in wi)
            assert r['words'] == env.tokenizer.decode_sentence(wi, break_on_eos=True, join=False)
            assert np.isfinite(r['score'])
            ids.update(wi)
        assert len(ids) > 5
        spk.wide_sample = False                                        # the switch is read at every pass
        with pytest.raises(NotImplementedError, match='wide_sample'):
            spk.test(feedback='sample')
    finally:
        random.setstate(rng_state)
        enc.eval()
        dec.eval()
