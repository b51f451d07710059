"""The cost of the path-fidelity metrics (SPL, nDTW, SDTW) on the g10 world (156 instructions on the five committed
scans: the world of tests/test_gpu_evaluation.py), in one process, after a warm-up, taking turns:

* Evaluation.score_agent with path_metrics off (sf_eval_score behind every rollout) and on (sf_eval_score_routes in its
  sweep layout): median of 12 with min / max;
* 16 x 156 recorded routes scored candidate by candidate with _score_item (what run_rational_follower(compute_oracle=True)
  did per minibatch) and as one batch with score_routes (one ragged launch), for both result types: median of 5.

    python tools/path_metrics_time.py [--out profiles/path_metrics_sweep.txt]

--coverage takes a third turn in both parts with coverage_metrics on (CLS: sf_eval_score_routes_coverage, the same launch
plus `near`, and one more download behind the same sync) under the name `cls`, and ends with the device time of the
kernel's two instantiations (sf_profile_begin / sf_profile_end) over the recorded routes and over the sweep:

    python tools/path_metrics_time.py --coverage [--out profiles/coverage_metrics_sweep.txt]"""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch                                                                 # noqa: E402
import r2r_world                                                             # noqa: E402
from speaker_follower_amd import agents, evaluation, features, model, nav, synth   # noqa: E402

REPS, ROUTE_REPS, COPIES = 12, 5, 16
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
coverage = '--coverage' in sys.argv
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


items, gold = r2r_world.load()
cfg = gold['config']
env, table, graphs = r2r_world.build_env(items, cfg, dense=False)
d = synth.FULL
enc_w, dec_w = synth.follower_weights_peaky(cfg['weight_seed'])
enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
enc.cuda().eval()
dec.cuda().eval()
agent = agents.Seq2SeqAgent(env, '/tmp/sf_path_metrics_time.json', enc, dec, episode_len=cfg['episode_len'])
agent.store = features.FeatureStore(table)
agent.use_device_env(nav.NavTable(env, agent.store))
evs = {'off': evaluation.Evaluation(env=env), 'on': evaluation.Evaluation(env=env, path_metrics=True)}
if coverage:
    evs['cls'] = evaluation.Evaluation(env=env, coverage_metrics=True)
data0, state0 = list(env.data), random.getstate()


def rewind():
    env.data[:] = data0
    random.setstate(state0)


times = {name: [] for name in evs}
summaries = {}
for rep in range(REPS + 2):                                                  # (the first two of each: warm-up, captures)
    for name in evs:
        rewind()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        summaries[name] = evs[name].score_agent(agent)[0]
        dt = time.perf_counter() - t0                                        # (score_agent ends in its host sync)
        if rep >= 2:
            times[name].append(dt * 1e3)
rewind()
for name in evs:
    assert evs[name].fallbacks == 0 and evs[name].last_host_syncs == 1
    ms = times[name]
    say('Evaluation.score_agent, path_metrics %-3s  median %.2f ms  min %.2f  max %.2f  (%d runs, %d instructions, %d '
        'minibatches of %d)' % (name, statistics.median(ms), min(ms), max(ms), REPS, len(items), len(agent.losses),
                                cfg['batch']))
for k in summaries['off']:
    assert summaries['on'][k] == summaries['off'][k], k
if coverage:
    for k in summaries['on']:
        assert summaries['cls'][k] == summaries['on'][k], k
    say('cls %.4f' % summaries['cls']['cls'])
say('spl %.4f  ndtw %.4f  sdtw %.4f  at success_rate %.4f' % tuple(summaries['on'][k] for k in
                                                                   ('spl', 'ndtw', 'sdtw', 'success_rate')))

results = {k: [(v, h, 0.0) for v, h in zip(w['viewpoints'], w['headings'])] for k, w in gold['items'].items()}
ids = [k for k in results if k in evs['on'].instr_ids] * COPIES
paths = [results[k] for k in ids]
for name in evs:
    ev = evs[name]
    ev.score_routes(ids, paths)
    loop, batch = [], []
    for rep in range(ROUTE_REPS):
        t0 = time.perf_counter()
        one_by_one = [ev._score_item(k, p) for k, p in zip(ids, paths)]
        loop.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        at_once = ev.score_routes(ids, paths)                                # (ends in its host sync)
        batch.append((time.perf_counter() - t0) * 1e3)
        assert [tuple(x) for x in one_by_one] == [tuple(x) for x in at_once]
    say('%d routes, path_metrics %-3s  _score_item per route: median %.1f ms   score_routes (one launch): median %.1f ms'
        '  (%d runs)' % (len(ids), name, statistics.median(loop), statistics.median(batch), ROUTE_REPS))
if coverage:                                                                 # the two instantiations of the one kernel
    from speaker_follower_amd import _lib
    with _lib.kernel_profile() as prof:
        for rep in range(ROUTE_REPS):
            for name in ('on', 'cls'):
                evs[name].score_routes(ids, paths)
    for kernel, row in sorted(prof.rows.items()):
        say('%d routes, kernel %-30s  avg %.1f us  min %.1f  max %.1f  (%d launches, taking turns)'
            % (len(ids), kernel, row['avg_us'], row['min_us'], row['max_us'], row['calls']))
    with _lib.kernel_profile() as prof:
        for rep in range(ROUTE_REPS):
            for name in ('on', 'cls'):
                rewind()
                evs[name].score_agent(agent)
    rewind()
    for kernel, row in sorted(prof.rows.items()):
        if 'eval_routes_kernel' in kernel:
            say('sweep of %d routes per launch, kernel %-30s  avg %.1f us  min %.1f  max %.1f  (%d launches)'
                % (cfg['batch'], kernel, row['avg_us'], row['min_us'], row['max_us'], row['calls']))
if out_path:
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
