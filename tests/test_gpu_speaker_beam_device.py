"""GPU: the speaker's beam search with its word loop on the device (Seq2SeqSpeaker.beam_on_device,
search.DeviceSpeakerBeam, sf_speaker_beam_select) against the reference's outputs (goldens G7 and G13) and, bit for bit,
against the host word loop (frontier.speaker_beam_search) run over the same number of decoder rows."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import search_world as W          # noqa: E402

SCORE_TOL = 3e-4                  # test_gpu_search.py: a score is a sum of <= 12 log-probabilities


def make_speaker(env, seed, words, peaky, episode_len=W.EPISODE_LEN):
    from speaker_follower_amd import model, agents, synth
    d = synth.FULL
    senc_w, sdec_w = (synth.speaker_weights_peaky if peaky else synth.speaker_weights)(seed)
    senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    senc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    sdec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    return agents.Seq2SeqSpeaker(env, '/tmp/sf_beam_dev_spk.json', senc.cuda().eval(), sdec.cuda().eval(), words,
                                 max_episode_len=episode_len)


def assert_identical(got, want):
    assert len(got) == len(want)
    for gl, wl in zip(got, want):
        assert len(gl) == len(wl)
        for g, w in zip(gl, wl):
            for key in ('instr_id', 'word_indices', 'score', 'scores', 'words'):
                assert g[key] == w[key], key
            assert len(g['attentions']) == len(w['attentions'])
            for a, b in zip(g['attentions'], w['attentions']):
                assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'g7_search.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def small():
    """The G7 world and speaker (test_gpu_search.py), one minibatch of its gold paths."""
    env, _ = W.build_world(dense=True)
    speaker = make_speaker(env, W.SPEAKER_SEED, W.INSTRUCTION_LEN, peaky=False)
    env.reset_epoch()
    path_obs, path_actions, _ = env.gold_obs_actions_and_instructions(W.EPISODE_LEN)
    return env, speaker, path_obs, path_actions


@pytest.fixture(scope='module')
def augmentation():
    """data_augmentation_from_speaker.py's shape: 20 paths, 40 candidates, 80 words, peaky weights."""
    env, _ = W.build_world(dense=True, n_items=20, batch=20, item_seed=7)
    speaker = make_speaker(env, 202, 80, peaky=True, episode_len=10)
    env.reset_epoch()
    path_obs, path_actions, _ = env.gold_obs_actions_and_instructions(10)
    return speaker, path_obs, path_actions


@pytest.mark.parametrize('beam', [1, 4])
def test_device_beam_matches_reference_g7(small, golden, beam):
    _, speaker, path_obs, path_actions = small
    speaker.beam_on_device = True
    fallbacks = speaker.beam_fallbacks
    try:
        outs = speaker.beam_search(beam, path_obs, path_actions)
    finally:
        speaker.beam_on_device = False
    assert speaker.beam_fallbacks == fallbacks and speaker.device_beam is not None
    want = golden['speaker_beam'][str(beam)]
    assert len(outs) == len(want)
    for ol, wl in zip(outs, want):
        assert len(ol) == len(wl)
        for o, w in zip(ol, wl):
            assert o['instr_id'] == w['instr_id']
            assert o['word_indices'] == w['word_indices']
            assert abs(o['score'] - w['score']) <= SCORE_TOL * max(1.0, abs(w['score']))
            np.testing.assert_allclose(o['scores'], w['scores'], rtol=2e-4, atol=2e-4)
            assert len(o['attentions']) == len(o['word_indices'])


def test_device_beam_rational_speaker_matches_reference_g13():
    """rational_speaker.py:9-137 with the speaker's beam search on the device: golden G13 as
    test_gpu_search.py::test_rational_speaker_pipeline_matches_reference checks it."""
    from speaker_follower_amd import model, features, agents, synth, search
    with open(os.path.join(HERE, 'golden', 'g13_rational_speaker.json')) as f:
        gold = json.load(f)
    cfg = gold['config']
    env, table = W.build_world(dense=True)
    d = synth.FULL
    enc_w, dec_w = synth.follower_weights_peaky(cfg['follower_seed'])
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    enc.cuda().eval()
    dec.cuda().eval()
    follower = agents.Seq2SeqAgent(env, '/tmp/sf_rs_dev.json', enc, dec, episode_len=cfg['episode_len'],
                                   max_instruction_length=cfg['instruction_len'])
    follower.store = features.FeatureStore(table)
    speaker = make_speaker(env, cfg['speaker_seed'], cfg['instruction_len'], peaky=True,
                           episode_len=cfg['episode_len'])
    speaker.store = follower.store
    speaker.beam_on_device = True
    by_id = search.generate_and_score_candidates(env, speaker, follower, cfg['n_candidates'])
    assert speaker.beam_fallbacks == 0 and speaker.device_beam.minibatches > 0
    assert {str(k) for k in by_id} == set(gold['candidates'])
    worst_s = worst_f = 0.0
    for k, lst in by_id.items():
        want = gold['candidates'][str(k)]
        assert len(lst) == len(want)
        for c, w in zip(lst, want):
            assert [int(x) for x in c['word_indices']] == w['word_indices']
            assert [int(a) for a in c['actions']] == w['actions']
            worst_s = max(worst_s, abs(c['speaker_score'] - w['speaker_score']) / max(1.0, abs(w['speaker_score'])))
            worst_f = max(worst_f, abs(c['follower_score'] - w['follower_score']) / max(1.0, abs(w['follower_score'])))
    print('device beam, rational speaker: worst relative score difference speaker %.2e, follower %.2e'
          % (worst_s, worst_f))
    assert worst_s <= SCORE_TOL and worst_f <= SCORE_TOL
    ss = np.array([c['speaker_score'] for lst in gold['candidates'].values() for c in lst])
    fs = np.array([c['follower_score'] for lst in gold['candidates'].values() for c in lst])
    res = search.predict_from_candidates(by_id, [float(w) for w in np.arange(0, 21) / 20.0])
    agree = total = 0
    for w, chosen in res.items():
        sw, fw = w / ss.std(), (1 - w) / fs.std()
        for k, best in chosen.items():
            want = gold['candidates'][str(k)]
            mixed = sorted((c['speaker_score'] * sw + c['follower_score'] * fw for c in want), reverse=True)
            got = next(i for i, c in enumerate(by_id[k]) if c is best)
            total += 1
            if got == gold['chosen']['%.2f' % w][str(k)]:
                agree += 1
            else:
                assert mixed[0] - mixed[1] <= 1e-3 * max(1.0, abs(mixed[0])), (w, k, mixed[:2])
    assert agree >= 0.97 * total


def test_device_beam_bit_exact_against_padded_host_loop(augmentation):
    """At the augmentation shape the device loop equals the host loop run over the same R = B * beam decoder rows: the
    same hypotheses in the same order, bit-identical scores, per-word scores and attention rows.  Against the unpadded
    host loop (its products see other row counts) the differences are reported."""
    from speaker_follower_amd import frontier, search
    speaker, path_obs, path_actions = augmentation
    B, beam = len(path_obs), 40
    dev = search.speaker_beam_search_device(speaker, beam, path_obs, path_actions)
    padded = frontier.speaker_beam_search(speaker, beam, path_obs, path_actions, pad_rows=B * beam)
    assert sum(len(x) for x in dev) == B * beam
    assert_identical(dev, padded)
    plain = frontier.speaker_beam_search(speaker, beam, path_obs, path_actions)
    differ, margin = 0, math.inf
    for d, p in zip(dev, plain):
        if [o['word_indices'] for o in d] != [o['word_indices'] for o in p] or [o['score'] for o in d] != \
                [o['score'] for o in p]:
            differ += 1
            sc = sorted({o['score'] for o in p}, reverse=True)
            if len(sc) > 1:
                margin = min(margin, min(a - b for a, b in zip(sc, sc[1:])))
    print('device beam vs the unpadded host loop: %d of %d instances differ; smallest score gap between neighbouring '
          'hypotheses of those: %s' % (differ, B, margin))


def test_device_beam_chunk_sizes_and_eager_issue_agree(augmentation):
    """Chunks of 1, 8 and T word steps, replayed or issued eagerly: identical outputs.  Host reads per minibatch at
    most ceil(T / chunk) + 1."""
    from speaker_follower_amd import search
    speaker, path_obs, path_actions = augmentation
    T, beam = speaker.instruction_len, 40
    ref = None
    for chunk, graphs in ((8, True), (1, True), (T, True), (8, False), (3, False)):
        outs = search.speaker_beam_search_device(speaker, beam, path_obs, path_actions, chunk=chunk, graphs=graphs)
        db = speaker.device_beam
        assert db.chunk == chunk and db.graphs == graphs
        assert db.last_host_reads <= math.ceil(T / chunk) + 1, (chunk, db.last_host_reads)
        print('chunk %d, graphs %s: %d host reads' % (chunk, graphs, db.last_host_reads))
        if ref is None:
            ref = outs
        else:
            assert_identical(outs, ref)


def test_wide_beam_falls_back_to_the_host_loop(small):
    _, speaker, path_obs, path_actions = small
    want = speaker.beam_search(65, path_obs, path_actions)
    before = speaker.beam_fallbacks
    speaker.beam_on_device = True
    try:
        got = speaker.beam_search(65, path_obs, path_actions)
    finally:
        speaker.beam_on_device = False
    assert speaker.beam_fallbacks == before + 1
    assert_identical(got, want)
