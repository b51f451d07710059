"""Seq2SeqSpeaker.beam_search (speaker.py:211-318) on the MI355X: milliseconds per minibatch of the host word loop
(frontier.speaker_beam_search: one blocking decoder step + top-k download + numpy selection per word) and of the device
word loop (search.DeviceSpeakerBeam: selection in sf_speaker_beam_select, chunks of word steps as replayed hipGraphs,
one live-count read per chunk), at the two shapes that drive it:
  * data_augmentation_from_speaker.py with a rational speaker: batch 20, 40 candidates, 80 words;
  * rational_speaker.py: batch 30, beam 10, 80 words.
Synthetic peaky speaker weights (synth.speaker_weights_peaky) over the fixture world of the search tests (three real
connectivity graphs, synthetic features).  The device path is timed only when the package has it.
Prints one JSON object.  python tools/speaker_beam_time.py [--reps N] [--chunk C] [--device-only] [--out FILE]"""
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


def speaker_for(env, seed=202, words=80, episode_len=10):
    from speaker_follower_amd import model, agents, synth
    d = synth.FULL
    senc_w, sdec_w = synth.speaker_weights_peaky(seed)
    senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    senc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    sdec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    return agents.Seq2SeqSpeaker(env, '/dev/null', senc.cuda().eval(), sdec.cuda().eval(), words,
                                 max_episode_len=episode_len)


def minibatches(B, n, seed=7):
    """n minibatches of B gold paths of the fixture world (observations with dense features, as beam_search takes)."""
    import search_world as W
    env, _ = W.build_world(dense=True, n_items=B * n, batch=B, item_seed=seed)
    env.reset_epoch()
    out = []
    for _ in range(n):
        path_obs, path_actions, _ = env.gold_obs_actions_and_instructions(10)
        out.append((path_obs, path_actions))
    return env, out


def time_path(speaker, batches, beam, on_device, reps):
    speaker.beam_on_device = on_device
    with torch.no_grad():
        for b in batches:                                       # warm-up (the device path: one graph per path length)
            speaker.beam_search(beam, *b)
        torch.cuda.synchronize()
        ms = []
        for i in range(reps):
            path_obs, path_actions = batches[i % len(batches)]
            t0 = time.perf_counter()
            outs = speaker.beam_search(beam, path_obs, path_actions)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
    out = dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)),
               hyps=sum(len(o) for o in outs))
    if on_device:        # the word loop with its one download; the rest is the encoder and the shared assembly
        out['word_loop_ms_last'] = speaker.device_beam.last_run_s * 1e3
        out['host_reads_last'] = speaker.device_beam.last_host_reads
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=6)
    ap.add_argument('--chunk', type=int, default=None, help='device path: word steps per replayed graph')
    ap.add_argument('--device-only', action='store_true', help='skip the host loop (e.g. under rocprofv3)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from speaker_follower_amd import agents
    have_device = hasattr(agents.Seq2SeqSpeaker, 'beam_on_device')
    res = dict(what='Seq2SeqSpeaker.beam_search, ms per minibatch (median of %d, after a warm-up pass)' % a.reps,
               device_path_available=have_device, shapes=[])
    for B, beam, words in ((20, 40, 80), (30, 10, 80)):
        env, batches = minibatches(B, 4)
        spk = speaker_for(env, words=words)
        row = dict(batch=B, beam=beam, words=words)
        if have_device and a.chunk is not None:
            spk.beam_chunk = a.chunk
        if not a.device_only:
            row['host'] = time_path(spk, batches, beam, False, a.reps)
        if have_device:
            row['device'] = time_path(spk, batches, beam, True, a.reps)
            row['device_fallbacks'] = spk.beam_fallbacks
            if 'host' in row:
                row['host_over_device'] = row['host']['ms_median'] / row['device']['ms_median']
        res['shapes'].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
