"""Seq2SeqAgent._score_obs_actions_and_instructions (follower.py:342-428: the follower's teacher-forced scoring of given
routes) on the MI355X: milliseconds per call of the per-step host loop (dense observations: a [rows, 36, 2176] float32
block plus the candidate rows stacked and uploaded per step, one blocking read per step) and of the device pass
(FollowerEngine over follower.route_index_batch's grids, chunks of SCORE_CHUNK rows, one download), and per minibatch
of search.generate_and_score_candidates (rational_speaker.py: speaker beam search + follower scoring of every
candidate along the gold route) with either, at the two shapes that drive it:
  * data_augmentation_from_speaker.py with a rational speaker: batch 20, 40 candidates;
  * rational_speaker.py: batch 30, 10 candidates.
Synthetic peaky weights over the fixture world of the search tests (three real connectivity graphs, synthetic
features); the speaker's word loop runs on the device in both columns (speaker.beam_on_device).
Prints one JSON object.  python tools/follower_route_scoring_time.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def agents_for(env, table, words=80, episode_len=10):
    from speaker_follower_amd import model, agents, synth, features
    d = synth.FULL
    enc_w, dec_w = synth.follower_weights_peaky(303)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    follower = agents.Seq2SeqAgent(env, '/dev/null', enc.cuda().eval(), dec.cuda().eval(), episode_len=episode_len)
    follower.store = features.FeatureStore(table)
    senc_w, sdec_w = synth.speaker_weights_peaky(202)
    senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    senc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    sdec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    speaker = agents.Seq2SeqSpeaker(env, '/dev/null', senc.cuda().eval(), sdec.cuda().eval(), words,
                                    max_episode_len=episode_len)
    speaker.store = follower.store
    speaker.beam_on_device = True
    return follower, speaker


def candidate_calls(env, speaker, n, K):
    """The follower scoring calls of n minibatches of generate_and_score_candidates: every candidate instruction of the
    speaker's beam along its gold route (rational_speaker.py:54-69), as (obs, actions, instructions)."""
    from speaker_follower_amd.follower import EOS
    env.reset_epoch()
    out = []
    with torch.no_grad():
        for _ in range(n):
            path_obs, path_actions, _ = env.gold_obs_actions_and_instructions(10)
            beams = speaker.beam_search(K, path_obs, path_actions)
            obs, acts, words = [], [], []
            for i, beam in enumerate(beams):
                for cand in beam:
                    idx = list(cand['word_indices'])
                    obs.append(path_obs[i])
                    acts.append(path_actions[i])
                    words.append(idx[:-1] if idx and idx[-1] == EOS else idx)
            out.append((obs, acts, words))
    return out


def ms_stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))


def time_scoring(follower, calls, on_device, reps):
    follower.score_on_device = on_device
    with torch.no_grad():
        for c in calls:                                         # warm-up
            follower._score_obs_actions_and_instructions(*c)
        torch.cuda.synchronize()
        ms = []
        for i in range(reps):
            c = calls[i % len(calls)]
            t0 = time.perf_counter()
            _, loss = follower._score_obs_actions_and_instructions(*c)
            float(loss)
            ms.append((time.perf_counter() - t0) * 1e3)
    out = ms_stats(ms)
    out['rows'] = len(calls[0][0])
    if on_device:
        out['host_reads_last'] = follower.last_host_reads
    return out


def time_pipeline(env, speaker, follower, K, on_device, reps):
    from speaker_follower_amd import search
    follower.score_on_device = on_device
    draws = []
    real = env.gold_obs_actions_and_instructions

    def counted(*a, **k):
        draws.append(1)
        return real(*a, **k)
    env.gold_obs_actions_and_instructions = counted
    try:
        search.generate_and_score_candidates(env, speaker, follower, K)      # warm-up
        ms = []
        for _ in range(reps):
            draws.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            search.generate_and_score_candidates(env, speaker, follower, K)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / len(draws))
    finally:
        env.gold_obs_actions_and_instructions = real
    return ms_stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import search_world as W
    res = dict(what='follower route scoring: ms per call, and generate_and_score_candidates: ms per minibatch '
                    '(median of %d, after a warm-up pass)' % a.reps, shapes=[])
    for B, K in ((20, 40), (30, 10)):
        env, table = W.build_world(dense=True, n_items=B, batch=B, item_seed=7)
        follower, speaker = agents_for(env, table)
        calls = candidate_calls(env, speaker, 2, K)
        row = dict(batch=B, candidates=K)
        row['scoring_host'] = time_scoring(follower, calls, False, a.reps)
        row['scoring_device'] = time_scoring(follower, calls, True, a.reps)
        row['scoring_host_over_device'] = row['scoring_host']['ms_median'] / row['scoring_device']['ms_median']
        row['minibatch_host'] = time_pipeline(env, speaker, follower, K, False, a.reps)
        row['minibatch_device'] = time_pipeline(env, speaker, follower, K, True, a.reps)
        row['minibatch_host_over_device'] = row['minibatch_host']['ms_median'] / row['minibatch_device']['ms_median']
        res['shapes'].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
