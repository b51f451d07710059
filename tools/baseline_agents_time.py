"""What a baseline agent's evaluation costs on the g10b world (the 782 instructions of R2R_sub_val_seen, batches of 100:
the world of tests/test_gpu_baseline_agents.py), in one process, after a warm-up, taking turns, per agent:

* `Evaluation.score_agent(agent)`: one sf_nav_walk launch over the split, one sf_eval_score_routes launch, one sync;
* `agent.test()` on the device path (one sf_nav_walk launch and one sync per minibatch) + `score_results`;
* `agent.test()` on the host path (env.reset / observe / step in Python) + `score_results`.

Median of 12 with min / max.  Information: nothing is gated on it.

    python tools/baseline_agents_time.py [--out profiles/baseline_agents_sweep.txt]"""
import os
import random
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402
import r2r_val_seen as VS                                                    # noqa: E402
from speaker_follower_amd import agents, evaluation, nav                     # noqa: E402

REPS, BATCH, SEED = 12, 100, 17
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


items, _ = VS.load_items()
env, _, _ = VS.build_env(items, batch_size=BATCH)
table = nav.NavTable(env, types.SimpleNamespace(device=torch.device('cuda', 0)))
ev = evaluation.Evaluation(env=env)
on_device, on_host = {}, {}
for name in ('Stop', 'Shortest', 'Random'):
    on_device[name] = agents.BaseAgent.get_agent(name)(env, '')
    on_device[name].use_device_env(table)
    on_host[name] = agents.BaseAgent.get_agent(name)(env, '')
data0, state0 = list(env.data), random.getstate()


def rewind():
    env.data[:] = data0
    random.setstate(state0)
    np.random.seed(SEED)


def sweep(name):
    return ev.score_agent(on_device[name])[0]


def test_on_device(name):
    return ev.score_results(on_device[name].test())[0]


def test_on_host(name):
    return ev.score_results(on_host[name].test())[0]


TURNS = (('score_agent (one walk launch)   ', sweep), ('test() on the device + scoring  ', test_on_device),
         ('test() on the host + scoring    ', test_on_host))
say('python tools/baseline_agents_time.py   (one MI355X; %d instructions, minibatches of %d, median of %d, taking turns)'
    % (len(items), BATCH, REPS))
for name in on_device:
    times = {label: [] for label, _ in TURNS}
    summaries = []
    for rep in range(REPS + 1):                                              # (the first round warms up)
        for label, fn in TURNS:
            rewind()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            summaries.append(fn(name))
            times[label].append((time.perf_counter() - t0) * 1e3)
    assert all(s == summaries[0] for s in summaries)
    for label, _ in TURNS:
        t = times[label][1:]
        say('%-8s %s median %8.2f ms  min %8.2f  max %8.2f' % (name, label, statistics.median(t), min(t), max(t)))
    say('%-8s success_rate %.4f  nav_error %.3f  steps %.2f' % (name, summaries[0]['success_rate'],
                                                                summaries[0]['nav_error'], summaries[0]['steps']))
rewind()
if out_path:
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
