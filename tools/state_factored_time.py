"""Seq2SeqAgent.state_factored_search (follower.py:720-980) on the MI355X: milliseconds per minibatch of the host
iteration loop (frontier.state_factored_search: per iteration the input block into pinned memory, one graph with its two
copies, a stream synchronise and the native bookkeeping of sim/frontier_core.cpp) and of the device iteration loop
(search.DeviceStateFactored: bookkeeping in sf_state_factored_select, chunks of iterations as replayed hipGraphs, one
status read per chunk), at two shapes:
  * the BIG fixture world of the search tests: batch 64, K = 40 completions, 1 successor, episode length 8 (BASELINE
    config 5's size; "peaky" synthetic follower weights);
  * the small fixture world: batch 8, 4 completions, 2 successors, episode length 6.
A call is timed end to end (env.reset, the encoder, the search, the result lists) with a device synchronise before and
after; the switch off (the host loop) and on (the device loop at every chunk size) take turns, minibatch by minibatch,
after a warm-up pass of each.  Prints a table and one JSON object.
python tools/state_factored_time.py [--reps N] [--chunks 1,2,4,8,16] [--device-only] [--out FILE]"""
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


def follower_for(big):
    import search_world as W
    from speaker_follower_amd import model, features, agents, synth
    if big:
        env, table = W.build_world(dense=False, n_items=W.BIG_ITEMS, batch=W.BIG_BATCH, item_seed=W.BIG_ITEM_SEED)
        weights, episode_len, n_batches = synth.follower_weights_peaky(W.BIG_FOLLOWER_SEED), W.BIG_EPISODE_LEN, 1
    else:
        env, table = W.build_world(dense=False)
        weights, episode_len, n_batches = synth.follower_weights(W.FOLLOWER_SEED), W.EPISODE_LEN, W.N_ITEMS // W.BATCH
    d = synth.FULL
    enc_w, dec_w = weights
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    agent = agents.Seq2SeqAgent(env, '/dev/null', enc.cuda().eval(), dec.cuda().eval(), episode_len=episode_len)
    agent.store = features.FeatureStore(table)
    return env, agent, n_batches


def one_call(agent, comp, succ, chunk):
    """chunk None: the switch off."""
    agent.search_on_device = chunk is not None
    if chunk is not None:
        agent.search_chunk = chunk
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        trajs, _, _ = agent.state_factored_search(comp, succ)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, sum(len(t) for t in trajs)


def summary(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)), runs=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--chunks', default='1,2,4,8,16', help='device loop: iterations per replayed graph')
    ap.add_argument('--device-only', action='store_true', help='skip the host loop (e.g. under rocprofv3)')
    ap.add_argument('--big-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    chunks = [int(c) for c in a.chunks.split(',')]
    paths = ([] if a.device_only else [('host', None)]) + [('device chunk %d' % c, c) for c in chunks]
    res = dict(what='Seq2SeqAgent.state_factored_search, ms per minibatch end to end (median of %d after a warm-up pass, '
                    'the paths taking turns)' % a.reps, shapes=[])
    lines = []
    for big, comp, succ in ((True, 40, 1), (False, 4, 2))[:1 if a.big_only else 2]:
        env, agent, n_batches = follower_for(big)
        env.set_beam_size(max(comp, succ))
        # one DeviceStateFactored per chunk size stays alive while the paths take turns
        caches = {}

        def call(chunk):
            if chunk is not None:
                agent.__dict__['_device_searches'] = caches.setdefault(chunk, {})
            return one_call(agent, comp, succ, chunk)

        for _, chunk in paths:                                    # warm-up: every minibatch once on every path
            env.reset_epoch()
            for _ in range(n_batches):
                call(chunk)
        ms = {name: [] for name, _ in paths}
        cands, loop_ms, info = {}, {name: [] for name, _ in paths}, {}
        for r in range(a.reps):
            for name, chunk in paths:                             # the same minibatch on each path, in turn
                env.reset_epoch()
                for _ in range(r % n_batches):
                    env.reset(sort=True, beamed=True)
                t, cands[name] = call(chunk)
                ms[name].append(t)
                if chunk is not None:
                    ds = agent.device_search
                    loop_ms[name].append(ds.last_run_s * 1e3)
                    info[name] = dict(iterations=ds.last_iterations, host_reads=ds.last_host_reads, chunk=ds.chunk)
        row = dict(batch=env.batch_size, completion_size=comp, successor_size=succ, episode_len=agent.episode_len,
                   fallbacks=agent.search_fallbacks, paths={})
        for name, chunk in paths:
            row['paths'][name] = dict(summary(ms[name]), candidates=cands[name])
            if chunk is not None:
                row['paths'][name].update(info[name], loop_ms_median=float(np.median(loop_ms[name])))
        res['shapes'].append(row)
        lines.append('batch %d, K = %d, %d successor(s), episode length %d  (fallbacks: %d)'
                     % (env.batch_size, comp, succ, agent.episode_len, agent.search_fallbacks))
        lines.append('  %-16s %9s  %-19s %11s %6s %6s %8s' % ('path', 'median ms', '(min - max)', 'loop median',
                                                             'iters', 'reads', 'vs host'))
        host = row['paths'].get('host', {}).get('ms_median')
        for name, chunk in paths:
            p = row['paths'][name]
            lines.append('  %-16s %9.2f  (%7.2f - %7.2f) %11s %6s %6s %8s' % (
                name, p['ms_median'], p['ms_min'], p['ms_max'],
                '%.2f' % p['loop_ms_median'] if chunk is not None else '',
                p.get('iterations', ''), p.get('host_reads', ''),
                '%.3f' % (p['ms_median'] / host) if host and chunk is not None else ''))
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(res['what'] + '\n' + text + '\n')


if __name__ == '__main__':
    main()
