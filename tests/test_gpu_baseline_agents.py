"""GPU: the baseline agents on their device path (ONE sf_nav_walk launch per rollout) and `Evaluation.score_agent` for
them (one walk launch + one route-scoring launch + one host sync for the whole split), on the val-seen world of G17.

* device-path agents == the fixture's 3 x 782 reference trajectories == the host-path agents;
* score_agent(agent) == agent.test() + score_results(agent.results) under the default, path_metrics and
  coverage_metrics evaluators, last_host_syncs == 1, fallbacks unchanged, env.ix / random / np.random where test()
  leaves them;
* ShortestAgent: success, cls == 1.0 and spl == 1.0 on every item whose gold path is the shortest path (per the fixture);
* a Seq2SeqAgent still sweeps as it did: the G10 world's score_agent == test() + score_results, default and path_metrics."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import r2r_val_seen as VS                                           # noqa: E402
import r2r_world                                                    # noqa: E402
import test_baseline_agents_host as H                               # noqa: E402
import test_gpu_evaluation as TE                                    # noqa: E402

DEV = torch.device('cuda', 0)
AGENTS = H.AGENTS
SWITCHES = {'default': {}, 'path': dict(path_metrics=True), 'coverage': dict(coverage_metrics=True)}


class Rewind(H.Rewind):
    """+ numpy's global stream, and where all three and env.ix stand after a walk."""

    def __init__(self, env, seed):
        H.Rewind.__init__(self, env)
        self.seed = seed

    def __call__(self):
        H.Rewind.__call__(self)
        np.random.seed(self.seed)

    def after(self):
        s = np.random.get_state()
        return self.env.ix, [it['instr_id'] for it in self.env.data], random.getstate(), s[1].tolist(), s[2:]


@pytest.fixture(scope='module')
def world():
    from speaker_follower_amd import agents, evaluation, nav
    gold = H.load_golden()
    items, _ = VS.load_items()
    env, _, _ = VS.build_env(items, batch_size=gold['config']['batch'])
    table = nav.NavTable(env, types.SimpleNamespace(device=DEV))
    made = {}
    for name in AGENTS:
        made[name] = agents.BaseAgent.get_agent(name)(env, '')      # (before the Rewind: BaseAgent seeds `random`)
        made[name].use_device_env(table)
        assert made[name]._device_table() is table
    return dict(gold=gold, env=env, table=table, agents=made, rewind=Rewind(env, gold['config']['seed']),
                evs={k: evaluation.Evaluation(env=env, **kw) for k, kw in SWITCHES.items()}, by_test={})


def by_test(w, name):
    """agent.test() on the device path, once per agent: (results as plain dictionaries, where the walk ended)."""
    if name not in w['by_test']:
        w['rewind']()
        results = w['agents'][name].test()
        end = w['rewind'].after()
        w['by_test'][name] = (results, end)
        w['rewind']()
    return w['by_test'][name]


@pytest.mark.parametrize('name', AGENTS)
def test_device_path_agents_reproduce_the_reference_and_the_host_path(world, name):
    from speaker_follower_amd import agents, nav
    results, _ = by_test(world, name)
    gold = world['gold']
    assert len(results) == 782
    for iid, res in results.items():
        assert isinstance(res, nav._WalkResult) and res.nav_rows()[0] is world['table']
        assert res['trajectory'] == H.golden_trajectory(gold, name, iid), iid        # (==: the floats too)
        assert set(res) == {'instr_id', 'trajectory'} and res['instr_id'] == iid
    host = agents.BaseAgent.get_agent(name)(world['env'], '')
    assert host._device_table() is None
    world['rewind']()
    want = host.test()
    world['rewind']()
    assert list(want) == list(results) and all(dict(results[k]) == want[k] for k in want)


@pytest.mark.parametrize('switch', list(SWITCHES))
@pytest.mark.parametrize('name', AGENTS)
def test_score_agent_equals_test_plus_score_results(world, name, switch):
    agent, ev, rewind = world['agents'][name], world['evs'][switch], world['rewind']
    results, end = by_test(world, name)
    summary, scores = ev.score_results(results)
    scores = {k: list(v) for k, v in scores.items()}
    fallbacks, sweeps = ev.fallbacks, ev.sweeps
    rewind()
    got_summary, got_scores = ev.score_agent(agent)
    assert rewind.after() == end                                      # env.ix, the item order, random, np.random
    assert ev.last_host_syncs == 1 and ev.fallbacks == fallbacks and ev.sweeps == sweeps + 1
    assert agent.results == {} and agent.losses == []
    assert set(got_scores) == set(scores) and len(got_scores['nav_errors']) == 780
    for k in scores:
        assert list(got_scores[k]) == scores[k], k                    # (== on floats: to the last bit, in the same order)
    assert got_summary == summary and 'model_score' not in summary
    assert ('spl' in summary) == (switch != 'default') and ('cls' in summary) == (switch == 'coverage')
    # keep_results: test()'s result objects from the same sync
    rewind()
    kept, _ = ev.score_agent(agent, keep_results=True)
    assert kept == summary and ev.last_host_syncs == 1
    assert list(agent.results) == list(results) and all(agent.results[k] == results[k] for k in results)
    agent.results = {}
    rewind()


def test_shortest_agent_is_perfect_wherever_the_gold_path_is_the_shortest_path(world):
    gold, ev = world['gold'], world['evs']['coverage']
    by_id = {it['instr_id']: it for it in world['env'].data}
    shortest_is_gold = {k for k, it in gold['agents']['Shortest']['items'].items()
                        if [gold['viewpoints'][v] for v in it['vp']] == by_id[k]['path']}
    assert len(shortest_is_gold) > 700                                # (the expectation comes from the fixture)
    world['rewind']()
    _, scores = ev.score_agent(world['agents']['Shortest'], keep_results=True)
    order = [k for k in world['agents']['Shortest'].results if k in ev.instr_ids]
    world['agents']['Shortest'].results = {}
    world['rewind']()
    hit = [i for i, k in enumerate(order) if k in shortest_is_gold]
    assert len(hit) >= 700
    for i in hit:
        assert scores['success'][i] is True and scores['cls'][i] == 1.0 and scores['spl'][i] == 1.0, order[i]
    if len(hit) == len(order):
        assert np.average(scores['success']) == 1.0


def test_a_table_that_is_not_on_the_device_takes_test(world):
    from speaker_follower_amd import agents
    ev = world['evs']['default']
    host = agents.StopAgent(world['env'], '')
    results, _ = by_test(world, 'Stop')
    world['rewind']()
    before = ev.fallbacks
    summary, _ = ev.score_agent(host)
    world['rewind']()
    assert ev.fallbacks == before + 1 and summary == ev.score_results(results)[0]
    assert len(host.results) == 782


def test_seq2seq_agents_sweep_as_they_did():
    """The G10 world of tests/test_gpu_evaluation.py: score_agent == test() + score_results, one host sync, no fallback,
    under the default evaluator and with path_metrics."""
    from speaker_follower_amd import evaluation, features, nav, synth
    items, gold = r2r_world.load()
    cfg = gold['config']
    env, table, _ = r2r_world.build_env(items, cfg, dense=False)
    store = features.FeatureStore(table)
    agent = TE.make_agent(env, store, synth.follower_weights_peaky(cfg['weight_seed']), cfg['episode_len'])
    agent.use_device_env(nav.NavTable(env, store))
    rewind = TE.Rewind(env)
    for kw in ({}, dict(path_metrics=True)):
        ev = evaluation.Evaluation(env=env, **kw)
        results = agent.test(use_dropout=False, feedback='argmax')
        summary, scores = ev.score_results(results)
        scores, losses, end = {k: list(v) for k, v in scores.items()}, list(agent.losses), rewind.after()
        rewind()
        got_summary, got_scores = ev.score_agent(agent)
        assert rewind.after() == end and ev.last_host_syncs == 1 and ev.fallbacks == 0 and ev.sweeps == 1
        assert got_summary == summary and agent.losses == losses
        for k in scores:
            assert list(got_scores[k]) == scores[k], k
        rewind()
    np.testing.assert_allclose(summary['success_rate'], gold['summary']['success_rate'], rtol=1e-9)
