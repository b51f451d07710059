"""Seq2SeqAgent.beam_search (follower.py:541-718) on the MI355X: milliseconds per minibatch of the host step loop
(frontier.beam_search: per decode step numpy table look-ups, an upload, ~25 launches, a blocking download and a numpy
selection) and of the device step loop (search.DeviceFollowerBeam: selection in sf_follower_beam_select, chunks of
decode steps as replayed hipGraphs, one live-count read per chunk), at two shapes:
  * batch 64, beam 40 (the shape DESIGN.md quotes for beam_search(K = 40));
  * batch 30, beam 10 (the rational follower's defaults).
Synthetic peaky follower weights (synth.follower_weights_peaky) over the fixture world of the search tests (three real
connectivity graphs, synthetic features, index-form observations), episode length 10.  A call is timed end to end
(env.reset, the encoder, the search, the result lists) with a device synchronise before and after; the two paths take
turns, minibatch by minibatch, after a warm-up pass of each.  The device path is timed only when the package has it.
Prints one JSON object.  python tools/follower_beam_time.py [--reps N] [--chunk C] [--device-only] [--out FILE]"""
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

EPISODE_LEN = 10


def follower_for(B, n_batches, seed=303, item_seed=15):
    import search_world as W
    from speaker_follower_amd import model, features, agents, synth
    env, table = W.build_world(dense=False, n_items=B * n_batches, batch=B, item_seed=item_seed)
    d = synth.FULL
    enc_w, dec_w = synth.follower_weights_peaky(seed)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    agent = agents.Seq2SeqAgent(env, '/dev/null', enc.cuda().eval(), dec.cuda().eval(), episode_len=EPISODE_LEN)
    agent.store = features.FeatureStore(table)
    return env, agent


def one_call(agent, beam, on_device):
    agent.beam_on_device = on_device
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        trajs, _, _ = agent.beam_search(beam)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, sum(len(t) for t in trajs)


def summary(ms):
    q1, q3 = np.percentile(ms, [25, 75])
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)),
                ms_q1=float(q1), ms_q3=float(q3), runs=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--chunk', type=int, default=None, help='device path: decode steps per replayed graph')
    ap.add_argument('--device-only', action='store_true', help='skip the host loop (e.g. under rocprofv3)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from speaker_follower_amd import agents
    have_device = hasattr(agents.Seq2SeqAgent, 'beam_on_device')
    paths = ([] if a.device_only else [('host', False)]) + ([('device', True)] if have_device else [])
    res = dict(what='Seq2SeqAgent.beam_search, ms per minibatch end to end (median of %d after a warm-up pass, the '
                    'paths taking turns)' % a.reps, device_path_available=have_device, episode_len=EPISODE_LEN, shapes=[])
    n_batches = 4
    for B, beam in ((64, 40), (30, 10)):
        env, agent = follower_for(B, n_batches)
        env.set_beam_size(beam)
        if have_device and a.chunk is not None:
            agent.beam_chunk = a.chunk
        row = dict(batch=B, beam=beam)
        for name, on in paths:                                    # warm-up: every minibatch once on every path
            env.reset_epoch()
            for _ in range(n_batches):
                one_call(agent, beam, on)
        ms = {name: [] for name, _ in paths}
        hyps, loop_ms = {}, []
        for r in range(a.reps):
            for name, on in paths:                                # the same minibatch on each path, in turn
                env.reset_epoch()
                for _ in range(r % n_batches):
                    env.reset(sort=True, beamed=True)
                t, hyps[name] = one_call(agent, beam, on)
                ms[name].append(t)
                if on:
                    loop_ms.append(agent.device_beam.last_run_s * 1e3)
        for name, _ in paths:
            row[name] = dict(summary(ms[name]), hyps=hyps[name])
        if 'device' in row:         # the step loop with its one download; the rest is the encoder and the shared assembly
            row['device']['step_loop_ms_median'] = float(np.median(loop_ms))
            row['device']['host_reads_last'] = agent.device_beam.last_host_reads
            row['device']['chunk'] = agent.device_beam.chunk
            row['device_fallbacks'] = agent.beam_fallbacks
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
