"""CPU: the baseline agents (agents.StopAgent / ShortestAgent / RandomAgent, follower.py:197-259) on their host path,
against G17 -- the reference's own agents on the reference's R2RBatch over all 782 instructions of R2R_sub_val_seen
(tests/golden/make_golden_baselines.py) -- and the numpy mirror of sf_nav_walk (tests/nav_walk_cases.py) against them,
so that the mirror is pinned before the kernel is held to it (tests/test_gpu_nav_walk.py)."""
import gzip
import importlib
import json
import os
import random
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nav_walk_cases as W                                          # noqa: E402
import r2r_val_seen as VS                                           # noqa: E402

ROOT = os.path.dirname(HERE)
AGENTS = ('Stop', 'Shortest', 'Random')
POLICY = dict(Stop=(W.STOP, 1), Shortest=(W.SHORTEST, 20), Random=(W.RANDOM, 6))
SUMMARY = ('nav_error', 'oracle_error', 'steps', 'lengths', 'success_rate', 'oracle_rate')


def load_golden():
    return json.load(gzip.open(os.path.join(VS.GOLDEN, 'g17_baseline_agents.json.gz'), 'rt'))


def golden_trajectory(gold, name, iid):
    it = gold['agents'][name]['items'][iid]
    return [(gold['viewpoints'][v], h, e) for v, h, e in zip(it['vp'], it['heading'], it['elevation'])]


class Rewind:
    """The environment's item order and `random` as they were: every walk starts from the same state."""

    def __init__(self, env):
        self.env, self.data, self.state = env, list(env.data), random.getstate()

    def __call__(self):
        self.env.data[:] = self.data
        random.setstate(self.state)


@pytest.fixture(scope='module')
def world():
    """The val-seen env at the fixture's batch size, its table on the CPU, and the three host-path walks, made once."""
    from speaker_follower_amd import agents, evaluation, nav
    gold = load_golden()
    items, _ = VS.load_items()
    env, _, _ = VS.build_env(items, batch_size=gold['config']['batch'])
    env.splits = ['sub_val_seen']
    rewind = Rewind(env)
    table = nav.NavTable(env, types.SimpleNamespace(device=torch.device('cpu')))
    results = {}
    for name in AGENTS:
        rewind()
        agent = agents.BaseAgent.get_agent(name)(env, '')
        assert agent._device_table() is None                          # (a host table or none at all: the host path)
        if name == 'Random':
            np.random.seed(gold['config']['seed'])
        results[name] = {k: dict(r) for k, r in agent.test().items()}
    rewind()
    return dict(gold=gold, env=env, rewind=rewind, table=table, results=results, ev=evaluation.Evaluation(env=env))


def test_the_header_declares_the_entry_and_the_library_binds_it():
    from speaker_follower_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'sf_hip.h')).read()
    assert re.search(r'\bint sf_nav_walk\(const sf_nav_table\* nav, int policy, int B, int S,', text)
    for name, value in (('STOP', 0), ('SHORTEST', 1), ('RANDOM', 2), ('RANDOM_MOVES', 5)):
        assert re.search(r'^#define SF_WALK_%s %d$' % (name, value), text, re.M), name
        assert getattr(_lib, 'SF_WALK_' + name) == value == getattr(W, name)
    assert 'sf_nav_walk' in _lib.EXPORTS and len(_lib.lib.sf_nav_walk.argtypes) == 16
    assert _lib.ABI_VERSION == 10                                     # (additive: the version stays)


def test_get_agent_resolves_the_three_names_and_no_fourth():
    from speaker_follower_amd import agents
    for name in AGENTS:
        cls = agents.BaseAgent.get_agent(name)
        assert cls is getattr(agents, name + 'Agent') and issubclass(cls, agents.BaseAgent)
    assert agents.BaseAgent.get_agent('Seq2Seq') is agents.Seq2SeqAgent
    with pytest.raises(KeyError):
        agents.BaseAgent.get_agent('Greedy')


def test_the_compat_modules_export_the_new_names():
    from speaker_follower_amd import agents, evaluation
    follower = importlib.import_module('speaker_follower_amd.compat.follower')
    ev = importlib.import_module('speaker_follower_amd.compat.eval')
    for name in AGENTS:
        assert getattr(follower, name + 'Agent') is getattr(agents, name + 'Agent')
    assert follower.BaseAgent.get_agent('Shortest') is agents.ShortestAgent
    assert ev.eval_simple_agents is evaluation.eval_simple_agents
    assert ev.evaluate_simple_agents is evaluation.evaluate_simple_agents


@pytest.mark.parametrize('name', AGENTS)
def test_host_path_agents_reproduce_the_reference_trajectories(world, name):
    gold, got = world['gold'], world['results'][name]
    assert gold['config']['n_items'] == 782 == len(got) == len(gold['agents'][name]['items'])
    assert gold['config']['numpy'].split('.')[0] == np.__version__.split('.')[0], 'RandomState streams are per numpy major'
    for iid, res in got.items():
        assert set(res) == {'instr_id', 'trajectory'} and res['instr_id'] == iid
        assert res['trajectory'] == golden_trajectory(gold, name, iid), iid          # (==: the floats too)


@pytest.mark.parametrize('name', AGENTS)
def test_score_results_reproduces_the_reference_numbers(world, name):
    """The standard tests/test_gpu_evaluation.py holds G10b to: counts and flags ==, distances to 1e-9 relative."""
    gold, ev = world['gold']['agents'][name], world['ev']
    summary, scores = ev.score_results(world['results'][name])
    order = [k for k in world['results'][name] if k in ev.instr_ids]
    assert len(order) == 780 == len(scores['nav_errors'])
    for i, k in enumerate(order):
        want = gold['items'][k]
        np.testing.assert_allclose([scores['nav_errors'][i], scores['oracle_errors'][i], scores['trajectory_lengths'][i]],
                                   [want['nav_error'], want['oracle_error'], want['length']], rtol=1e-9)
        assert (scores['trajectory_steps'][i], scores['success'][i], scores['oracle_success'][i]) == (
            want['steps'], want['success'], want['oracle_success']), k
    assert set(summary) == set(SUMMARY)
    for k in SUMMARY:
        np.testing.assert_allclose(summary[k], gold['summary'][k], rtol=1e-9)
    if name == 'Stop':
        assert summary['steps'] == 0 and summary['lengths'] == 0
    if name == 'Shortest':
        assert summary['success_rate'] == 1.0 and summary['nav_error'] == 0.0


def first_actions(table, rows, views):
    a_num = table.host['a_num'][rows.astype(np.int64) * 36 + views].tolist()
    return np.array([np.random.randint(n - 1) + 1 for n in a_num], np.int32)


@pytest.mark.parametrize('name', AGENTS)
def test_the_mirror_on_the_env_tables_equals_the_host_path(world, name):
    table, env, gold = world['table'], world['env'], world['gold']
    items = list(env.data)                                            # first occurrences come in data order
    policy, S = POLICY[name]
    rows, views = table.start_states(items)
    first = hop = base = None
    if name == 'Random':
        np.random.seed(gold['config']['seed'])
        first = first_actions(table, rows, views)
    if name == 'Shortest':
        hop, base = table.hop_rows(items)
    h = table.host
    tab = dict(a_num=h['a_num'], next_row=h['next_row'], cand_view=h['cand_view'], A=table.A, V=36)
    out = W.mirror_walk(tab, policy, S, rows, views, first, hop, base)
    assert out['err'] == 0
    inc = np.pi / 6
    for b, it in enumerate(items):
        n = int(out['n_steps'][b])
        poses = [(table.vp_of[out['row'][t, b]][1], (int(out['view'][t, b]) % 12) * inc,
                  (int(out['view'][t, b]) // 12 - 1) * inc) for t in range(n + 1)]
        assert poses == world['results'][name][it['instr_id']]['trajectory'], it['instr_id']
    # the table's own result objects say the same
    res = table.walk_results(items, out['row'], out['view'], out['n_steps'])
    assert all(r == world['results'][name][r['instr_id']] for r in res)
    assert [len(r.nav_rows()[1]) for r in res] == (out['n_steps'] + 1).tolist()


def minibatches_of_a_test(env):
    """The minibatches BaseAgent.test walks: reset() until an id repeats."""
    env.reset_epoch()
    seen, looped, out = set(), False, []
    while not looped:
        env.reset()
        out.append(list(env.batch))
        for it in env.batch:
            looped = looped or it['instr_id'] in seen
            seen.add(it['instr_id'])
    return out


def test_random_agent_draws_once_per_row_walked_at_every_batch_size(world):
    """One draw per observation in observation order, repeated ids included: numpy's stream ends where a replay of the
    walked minibatches over the table's candidate counts ends, and what an instruction gets does not depend on the
    batch size."""
    from speaker_follower_amd import agents
    env, table, rewind, seed = world['env'], world['table'], world['rewind'], world['gold']['config']['seed']
    size0 = env.batch_size
    try:
        for size in (1, 39, 100):
            env.batch_size = size
            agent = agents.RandomAgent(env, '')                        # (before the rewind: BaseAgent seeds `random`)
            rewind()
            np.random.seed(seed)
            got = agent.test()
            end, ix = np.random.get_state(), env.ix
            assert {k: dict(r) for k, r in got.items()} == world['results']['Random'], size
            rewind()
            np.random.seed(seed)
            walked = minibatches_of_a_test(env)
            assert len(walked) == -(-782 // size) + (782 % size == 0) and env.ix == ix
            for mb in walked:
                first_actions(table, *table.start_states(mb))
            replay = np.random.get_state()
            assert replay[2] == end[2] and (replay[1] == end[1]).all(), size
    finally:
        env.batch_size = size0
        rewind()


def test_random_agent_raises_as_the_reference_does(world):
    """A start state with one candidate: numpy's own ValueError from randint(0); a later dead end: AssertionError."""
    from speaker_follower_amd import agents
    env = world['env']
    agent = agents.RandomAgent(env, '')
    ob = dict(instr_id='x', viewpoint='v', heading=0.0, elevation=0.0, adj_loc_list=[{}])
    two = dict(ob, adj_loc_list=[{}, {}])
    calls = []
    fake = types.SimpleNamespace(reset=lambda: [None], step=lambda ws, a, obs: ws,
                                 observe=lambda ws: [two if not calls.append(1) and len(calls) == 1 else ob])
    agent.env = fake
    with pytest.raises(AssertionError):
        agent._rollout_on_host()
    agent.env = types.SimpleNamespace(reset=lambda: [None], observe=lambda ws: [ob])
    with pytest.raises(ValueError):
        agent._rollout_on_host()


def test_evaluate_simple_agents_writes_the_three_files_and_scores_them(world, tmp_path, capsys):
    from speaker_follower_amd import evaluation
    env, ev, rewind = world['env'], world['ev'], world['rewind']
    rewind()
    np.random.seed(3)
    out = evaluation.evaluate_simple_agents(env, ev, str(tmp_path) + os.sep)
    rewind()
    assert list(out) == list(AGENTS)
    assert sorted(os.listdir(tmp_path)) == sorted('sub_val_seen_%s_agent.json' % a.lower() for a in AGENTS)
    printed = capsys.readouterr().out
    for name in AGENTS:
        path = os.path.join(tmp_path, 'sub_val_seen_%s_agent.json' % name.lower())
        summary, _ = ev.score_file(path)
        assert summary == out[name] and set(summary) == set(SUMMARY)
        assert '\n%s\n' % name in printed
        written = json.load(open(path))
        assert len(written) == 782 and all(set(r) == {'instr_id', 'trajectory'} for r in written.values())
    # Stop and Shortest do not draw: their files hold the fixture's trajectories (tuples become lists in JSON)
    for name in ('Stop', 'Shortest'):
        written = json.load(open(os.path.join(tmp_path, 'sub_val_seen_%s_agent.json' % name.lower())))
        assert all(r['trajectory'] == [list(p) for p in world['results'][name][k]['trajectory']] for k, r in written.items())
