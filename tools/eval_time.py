"""Validation on val-seen (782 instructions, batch 100: the world of tests/test_gpu_r2r_val_seen.py) two ways in one
process, after a warm-up, taking turns: agent.test() then oracle.np_env.score_results with warm Dijkstra caches (how a
validation was scored before speaker_follower_amd.evaluation), and Evaluation.score_agent (one sweep, one host sync).
Median of 7 with min / max.  Also the one-off construction of the distance table: sf_eval_distances on the device
against NavGraph.shortest over the same 51 scans.

    python tools/eval_time.py [--out profiles/evaluation_sweep.txt]"""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402
import r2r_val_seen as VS                                                    # noqa: E402
from oracle import np_env                                                    # noqa: E402
from speaker_follower_amd import agents, env as env_mod, evaluation, features, model, nav, synth   # noqa: E402

REPS = 7
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


items, _ = VS.load_items()
gold = VS.load_sr_golden()
cfg = gold['config']
env, row_of, n_rows = VS.build_env(items, batch_size=cfg['batch'], table_seed=cfg['table_seed'], scans=cfg['scans'])
d = synth.FULL
enc_w, dec_w = synth.follower_weights_peaky(cfg['weight_seed'])
for k, v in gold['head'].items():
    dec_w[k] = np.asarray(v, np.float32).reshape(dec_w[k].shape)
enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
enc.cuda().eval()
dec.cuda().eval()
agent = agents.Seq2SeqAgent(env, '/tmp/sf_eval_time.json', enc, dec, episode_len=cfg['episode_len'])
agent.store = features.FeatureStore(env.host_table)
agent.use_device_env(nav.NavTable(env, agent.store))
gt = {it['path_id']: it for it in items}

# ---- the one-off construction: the table of the split's scans, device kernel against the host searches
scans = sorted({it['scan'] for it in items})
fresh = {s: env_mod.NavGraph(os.path.join(env.nav_graph_path, s + '_connectivity.json')) for s in scans}
torch.cuda.synchronize()
t0 = time.perf_counter()
on_dev = evaluation.DistanceTable(fresh, device='cuda')
torch.cuda.synchronize()
t_dev = time.perf_counter() - t0
fresh = {s: env_mod.NavGraph(os.path.join(env.nav_graph_path, s + '_connectivity.json')) for s in scans}
t0 = time.perf_counter()
on_host = evaluation.DistanceTable(fresh, device='cpu')
t_host = time.perf_counter() - t0
assert (on_dev.host == on_host.host).all()
say('distance table of %d scans (%d viewpoints, %.1f MB): sf_eval_distances + CSR + download %.1f ms; '
    'NavGraph.shortest from every viewpoint %.1f ms; bit-equal'
    % (len(scans), sum(on_dev.m.values()), on_dev.host.nbytes / 1e6, t_dev * 1e3, t_host * 1e3))

ev = evaluation.Evaluation(env=env)
data0, state0 = list(env.data), random.getstate()


def rewind():
    env.data[:] = data0
    random.setstate(state0)


def parent_way():
    results = agent.test(use_dropout=False, feedback='argmax')
    scored = {k: v for k, v in results.items() if k in ev.instr_ids}
    return np_env.score_results(gt, env.graphs, scored)[0]


def sweep():
    return ev.score_agent(agent)[0]


for fn in (parent_way, sweep, parent_way, sweep):                            # warm-up: captures, hop tables, Dijkstra caches
    rewind()
    first = fn()
times = {parent_way: [], sweep: []}
summaries = {}
for rep in range(REPS):
    for fn in (parent_way, sweep):
        rewind()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        summaries[fn] = fn()
        torch.cuda.synchronize()
        times[fn].append(time.perf_counter() - t0)
rewind()
assert ev.fallbacks == 0 and ev.last_host_syncs == 1
for k in ('nav_error', 'oracle_error', 'steps', 'lengths', 'success_rate', 'oracle_rate'):
    np.testing.assert_allclose(summaries[sweep][k], summaries[parent_way][k], rtol=1e-12)
for name, fn in (('agent.test() + oracle.np_env.score_results (warm caches)', parent_way),
                 ('Evaluation.score_agent (one sweep, one host sync)', sweep)):
    ms = [x * 1e3 for x in times[fn]]
    say('%-60s median %.2f ms  min %.2f  max %.2f  (%d runs, %d instructions, %d minibatches of %d)'
        % (name, statistics.median(ms), min(ms), max(ms), REPS, len(items), len(agent.losses), cfg['batch']))
say('success_rate %.6f both ways' % summaries[sweep]['success_rate'])
if out_path:
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
