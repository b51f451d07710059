#!/usr/bin/env python3
"""G17: the reference's baseline agents pinned on the split it ships -- BUILD container only.

The reference's `StopAgent`, `ShortestAgent` and `RandomAgent` (follower.py:197-259) walk the reference's `R2RBatch`
(tasks/R2R/env.py, over this repo's navigation-only simulator binary, set up exactly as make_golden_env.reference_env()
does for G15 and G10b) over ALL 782 instructions / 260 paths of tasks/R2R/data/R2R_sub_val_seen.json, through the
reference's own `BaseAgent.test()`; the reference's `Evaluation._score_item / score_results` (eval.py:56-139) score each
result.  `RandomAgent` draws from numpy's global stream: `np.random.seed(SEED)` immediately before its `test()`.

Writes tests/golden/g17_baseline_agents.json.gz (data only): config (split, batch, seeds, numpy version), the table of
viewpoint ids the trajectories index, and per agent the summary and per instruction the trajectory (viewpoint index,
heading, elevation) with the reference Evaluation's per-item numbers.
"""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_env import reference_env, _TinyFeatures           # noqa: E402

SPLIT, BATCH, ENV_SEED, SEED = 'sub_val_seen', 100, 10, 17
AGENTS = ('Stop', 'Shortest', 'Random')


def main():
    ref_env, ref_utils = reference_env()                              # (cwd is now the reference tree)
    import follower as ref_follower
    sys.argv = ['eval.py']
    import eval as ref_eval
    vocab = ref_utils.read_vocab(os.path.join('tasks', 'R2R', 'data', 'train_vocab.txt'))
    tok = ref_utils.Tokenizer(vocab=vocab)
    ev = ref_eval.Evaluation([SPLIT])

    vps, agents = {}, {}
    for name in AGENTS:
        # a fresh environment per agent: test() reshuffles the data when the epoch wraps
        env = ref_env.R2RBatch([_TinyFeatures()], batch_size=BATCH, seed=ENV_SEED, splits=[SPLIT], tokenizer=tok)
        agent = ref_follower.BaseAgent.get_agent(name)(env, '')
        if name == 'Random':
            np.random.seed(SEED)
        results = agent.test()
        assert len(results) == len(env.data) == 782
        summary, _ = ev.score_results(results)
        items = {}
        for iid, res in results.items():
            r = ev._score_item(iid, res['trajectory'])
            items[iid] = dict(vp=[vps.setdefault(p[0], len(vps)) for p in res['trajectory']],
                              heading=[float(p[1]) for p in res['trajectory']],
                              elevation=[float(p[2]) for p in res['trajectory']],
                              nav_error=float(r.nav_error), oracle_error=float(r.oracle_error),
                              steps=int(r.trajectory_steps), length=float(r.trajectory_length),
                              success=bool(r.success), oracle_success=bool(r.oracle_success))
        agents[name] = dict(summary={k: float(v) for k, v in summary.items()}, items=items)
        print(name, agents[name]['summary'])

    out = dict(config=dict(split=SPLIT, batch=BATCH, env_seed=ENV_SEED, seed=SEED, numpy=np.__version__, n_items=782),
               viewpoints=sorted(vps, key=vps.get), agents=agents)
    path = os.path.join(HERE, 'g17_baseline_agents.json.gz')
    with gzip.GzipFile(path, 'wb', compresslevel=9, mtime=0) as f:
        f.write(json.dumps(out, separators=(',', ':')).encode())
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
