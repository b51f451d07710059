"""CPU: speaker_follower_amd.evaluation (eval.py:23-139 in the package) against the reference Evaluation's recorded
numbers and against the test oracle's restatement.

* g10 (156 instructions, the five committed connectivity graphs) and g10b (782 instructions of the val-seen split,
  geometry from nav_data.connectivity_dir): plain result dictionaries built from the goldens' viewpoints / headings /
  score; per item within rtol 1e-9 of the reference's `Evaluation` (the bound of tests/test_oracle_golden.py; the
  reference's loader forms edge lengths with another expression, measured difference <= 3.6e-15), integers and flags equal.
* the same results through oracle.np_env.score_results over the same NavGraphs: per-item floats BIT-EQUAL (same
  distances, same order of additions), summary within rtol 1e-12 (np.average against np.mean of the same lists).
* the reference's contract: its two assertions, ids outside '<path>_0' .. '_2' ignored, score_file, the bare-name import,
  the split-file constructor.
* results of a device rollout are scored from their nav rows: no 'trajectory' is built.

Without a GPU the distance table comes from NavGraph.shortest; with one, from sf_eval_distances -- the same numbers."""
import json
import os
import random
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import r2r_world                                                    # noqa: E402
import r2r_val_seen as VS                                           # noqa: E402
from oracle import np_env                                           # noqa: E402

FLOATS = (('nav_errors', 'nav_error'), ('oracle_errors', 'oracle_error'), ('trajectory_lengths', 'length'))
EXACT = (('trajectory_steps', 'steps'), ('success', 'success'), ('oracle_success', 'oracle_success'))
SUMMARY = ('nav_error', 'oracle_error', 'steps', 'lengths', 'success_rate', 'oracle_rate')


def results_of(gold):
    out = {}
    for k, w in gold['items'].items():
        el = w.get('elevations', [0.0] * len(w['viewpoints']))
        out[k] = dict(instr_id=k, trajectory=[(v, h, e) for v, h, e in zip(w['viewpoints'], w['headings'], el)],
                      score=w['score'])
    return out


@pytest.fixture(scope='module')
def g10():
    from speaker_follower_amd import env, evaluation
    items, gold = r2r_world.load()
    graphs = {s: env.NavGraph(os.path.join(r2r_world.CONN, s + '_connectivity.json')) for s in gold['config']['scans']}
    return items, gold, graphs, evaluation.Evaluation(items=items, graphs=graphs)


@pytest.fixture(scope='module')
def g10b():
    from speaker_follower_amd import env, evaluation, nav_data
    items, _ = VS.load_items()
    gold = VS.load_sr_golden()
    scans = sorted({it['scan'] for it in items})
    conn = nav_data.connectivity_dir(scans=scans)
    graphs = {s: env.NavGraph(os.path.join(conn, s + '_connectivity.json')) for s in scans}
    return items, gold, graphs, evaluation.Evaluation(items=items, graphs=graphs)


@pytest.fixture(params=['g10', 'g10b'])
def world(request):
    return request.getfixturevalue(request.param)


def test_attributes_follow_the_reference(g10b):
    items, gold, graphs, ev = g10b
    assert ev.error_margin == 3.0
    assert set(ev.gt) == {it['path_id'] for it in items} and len(ev.gt) == 260
    assert ev.instr_ids == {'%d_%d' % (p, i) for p in ev.gt for i in range(3)} and len(ev.instr_ids) == 780
    assert ev.scans == {it['scan'] for it in items}
    from speaker_follower_amd import evaluation
    assert evaluation.EvalResult._fields == ('nav_error', 'oracle_error', 'trajectory_steps', 'trajectory_length',
                                             'success', 'oracle_success')


def test_scores_equal_the_reference_evaluation(world):
    items, gold, graphs, ev = world
    results = results_of(gold)
    summary, scores = ev.score_results(results)
    scored = [k for k in results if k in ev.instr_ids]
    assert len(scored) == len(ev.instr_ids) == len(scores['nav_errors'])
    worst = 0.0
    for mine, theirs in FLOATS:
        want = np.array([gold['items'][k][theirs] for k in scored])
        worst = max(worst, float(np.abs(np.array(scores[mine]) - want).max()))
        np.testing.assert_allclose(scores[mine], want, rtol=1e-9)
    print('largest absolute difference to the reference Evaluation: %.3g' % worst)
    for mine, theirs in EXACT:
        assert scores[mine] == [gold['items'][k][theirs] for k in scored], mine
    assert set(summary) == set(SUMMARY) | {'model_score'}
    for k in SUMMARY + ('model_score',):
        np.testing.assert_allclose(summary[k], gold['summary'][k], rtol=1e-9)
    if len(scored) == 780:
        assert summary['success_rate'] == 65 / 780
    else:
        assert summary['success_rate'] == 10 / 156


def test_scores_are_bit_equal_to_the_oracle_restatement(world):
    items, gold, graphs, ev = world
    results = {k: v for k, v in results_of(gold).items() if k in ev.instr_ids}
    summary, scores = ev.score_results(results)
    want_summary, per_item = np_env.score_results({it['path_id']: it for it in items}, graphs, results)
    for i, k in enumerate(results):
        w = per_item[k]
        got = (scores['nav_errors'][i], scores['oracle_errors'][i], scores['trajectory_lengths'][i])
        assert got == (w['nav_error'], w['oracle_error'], w['length']), k               # (==: to the last bit)
        assert (scores['trajectory_steps'][i], scores['success'][i], scores['oracle_success'][i]) == \
            (w['steps'], w['success'], w['oracle_success'])
        r = ev._score_item(k, results[k]['trajectory'])
        assert tuple(r) == got[:2] + (w['steps'], got[2], w['success'], w['oracle_success'])
    for k in SUMMARY:
        np.testing.assert_allclose(summary[k], want_summary[k], rtol=1e-12)


def test_the_table_keeps_the_source_major_orientation(g10):
    items, gold, graphs, ev = g10
    t = ev.table
    asym = unreachable = 0
    for s in t.scans:
        D, g = t.block(s), graphs[s]
        for i in (0, len(t.nodes[s]) // 2, len(t.nodes[s]) - 1):
            v = t.nodes[s][i]
            dist = g.shortest(v)[0]
            want = np.array([dist.get(u, np.inf) for u in t.nodes[s]])
            assert (D[i] == want).all()
            assert ev.distance(s, v, t.nodes[s][0]) == want[0]
        asym += int((D != D.T).sum())
        unreachable += int(np.isinf(D).sum())
    assert asym > 0                                      # D[a][b] and D[b][a] differ in their last bits: not symmetrised
    print('%d asymmetric entries, %d unreachable pairs on the five scans' % (asym, unreachable))


def test_a_missing_id_raises_the_references_assertion(g10):
    items, gold, graphs, ev = g10
    results = results_of(gold)
    results.pop(next(iter(results)))
    with pytest.raises(AssertionError, match='Missing 1 of 156 instruction ids'):
        ev.score_results(results)


def test_a_trajectory_that_does_not_start_at_the_start_raises(g10):
    items, gold, graphs, ev = g10
    results = results_of(gold)
    k = next(iter(results))
    results[k] = dict(results[k], trajectory=results[k]['trajectory'][1:] + [(items[0]['path'][-1], 0.0, 0.0)])
    assert results[k]['trajectory'][0][0] != ev.gt[int(k.split('_')[0])]['path'][0]
    with pytest.raises(AssertionError, match='should include the start position'):
        ev.score_results(results)


def test_ids_outside_the_three_per_path_are_ignored(g10b):
    items, gold, graphs, ev = g10b
    results = results_of(gold)
    extra = [k for k in results if int(k.split('_')[1]) >= 3]
    assert sorted(extra) == ['135_3', '568_3']
    summary, scores = ev.score_results(results)
    without, scores2 = ev.score_results({k: v for k, v in results.items() if k not in extra})
    assert len(scores['nav_errors']) == 780 and summary == without


def test_results_without_score_have_no_model_score(g10):
    items, gold, graphs, ev = g10
    results = {k: {'instr_id': k, 'trajectory': v['trajectory']} for k, v in results_of(gold).items()}
    summary, _ = ev.score_results(results)
    assert set(summary) == set(SUMMARY)


def test_score_file_round_trips_write_results(g10, tmp_path):
    from speaker_follower_amd import agents
    items, gold, graphs, ev = g10
    state = random.getstate()
    agent = agents.BaseAgent(None, str(tmp_path / 'results.json'))      # (seeds `random`, follower.py:114)
    random.setstate(state)
    agent.results = results_of(gold)
    agent.write_results()
    summary, scores = ev.score_file(agent.results_path)
    want, want_scores = ev.score_results({k: {'instr_id': k, 'trajectory': v['trajectory']}
                                          for k, v in agent.results.items()})
    assert summary == want and dict(scores) == dict(want_scores) and 'model_score' not in summary


def test_the_bare_name_import_and_the_split_file_constructor(g10, tmp_path, monkeypatch):
    from speaker_follower_amd import compat, evaluation
    items, gold, graphs, ev = g10
    monkeypatch.syspath_prepend(compat.path())
    sys.modules.pop('eval', None)
    import eval as bare
    try:
        assert bare.Evaluation is evaluation.Evaluation and bare.EvalResult is evaluation.EvalResult
    finally:
        sys.modules.pop('eval', None)
    # R2R_<split>.json in the reference's layout: one entry per PATH with its three instructions
    paths = {}
    for it in items:
        paths.setdefault(it['path_id'], dict(path_id=it['path_id'], scan=it['scan'], path=it['path'],
                                             heading=it['heading'], distance=it.get('distance', 0.0),
                                             instructions=['a', 'b', 'c']))
    (tmp_path / 'tasks' / 'R2R' / 'data').mkdir(parents=True)
    (tmp_path / 'tasks' / 'R2R' / 'data' / 'R2R_tiny.json').write_text(json.dumps(list(paths.values())))
    os.symlink(r2r_world.CONN, str(tmp_path / 'connectivity'))
    monkeypatch.chdir(tmp_path)
    ev2 = evaluation.Evaluation(['tiny'])
    assert ev2.splits == ['tiny'] and ev2.instr_ids == ev.instr_ids and ev2.scans == ev.scans
    results = results_of(gold)
    assert ev2.score_results(results)[0] == ev.score_results(results)[0]


class HostNav:
    """The row layout of nav.NavTable (scans sorted, included viewpoints in connectivity-file order) without its device
    tables: what a result of a device rollout refers to."""

    def __init__(self, graphs):
        self.vp_of, self.row_of, self.base, self.scan_rows = [], {}, {}, {}
        for s in sorted(graphs):
            nodes = [v for v, inc in zip(graphs[s].ids, graphs[s].included) if inc]
            self.base[s], self.scan_rows[s] = len(self.vp_of), len(nodes)
            for v in nodes:
                self.row_of[(s, v)] = len(self.vp_of)
                self.vp_of.append((s, v))


def test_device_rollout_results_are_scored_from_their_rows(g10, monkeypatch):
    from speaker_follower_amd import nav
    items, gold, graphs, ev = g10
    table = HostNav(graphs)
    S, B = gold['config']['episode_len'], len(items)
    rows, views = np.zeros((S + 1, B), np.int32), np.zeros((S + 1, B), np.int32)
    acts, sc = np.ones((S, B), np.int64), np.zeros((S, B), np.float32)
    for b, it in enumerate(items):
        vps = gold['items'][it['instr_id']]['viewpoints']
        n = len(vps) - 1
        r = [table.row_of[(it['scan'], v)] for v in vps]
        rows[:, b] = r + [r[-1]] * (S - n)
        if n < S:
            acts[n - 1, b] = 0                               # (a stop ended it)
        sc[:n, b] = gold['items'][it['instr_id']]['score'] / n
    made = []
    monkeypatch.setattr(nav._Trajectory, '_make', lambda self, key: made.append(key) or [])
    trajs = nav.DeviceNavBatch.trajectories_from(types.SimpleNamespace(nav=table), items, S, rows, views, acts, sc)
    results = {tr['instr_id']: tr for tr in trajs}
    summary, scores = ev.score_results(results)
    assert made == []                                        # no 'trajectory' was built
    plain = {k: v for k, v in results_of(gold).items()}
    plain = {k: dict(plain[k], score=results[k]['score']) for k in results}
    want, want_scores = ev.score_results(plain)
    assert dict(scores) == dict(want_scores)                 # (== on floats: to the last bit)
    assert summary == want and 'model_score' in summary
    # a result that starts elsewhere is refused on this path too
    rows[0, 0] = rows[0, 0] + 1
    bad = nav.DeviceNavBatch.trajectories_from(types.SimpleNamespace(nav=table), items, S, rows, views, acts, sc)
    with pytest.raises(AssertionError, match='should include the start position'):
        ev.score_results({tr['instr_id']: tr for tr in bad})
