"""CPU: the path-fidelity metrics of `evaluation.Evaluation(path_metrics=True)` -- SPL, nDTW, SDTW, which the reference
does not compute -- against their published definitions restated in tests/path_metric_cases.py, with ==.

* the known answers on the unit line graph;
* per item over the recorded trajectories of the g10 and g10b goldens (156 and 782 results): every per-item list, the
  summary keys, and the classic lists and summary values against a default Evaluation;
* the gold paths of val-seen scored as their own predictions: dtw 0.0, ndtw 1.0, spl 1.0 for all 260;
* the direction of the cost (D[pred][gold]), two components (dtw inf -> ndtw 0.0, no NaN), start == goal;
* the synthetic case list shared with the GPU file, through `_score_item`, `score_routes` and `score_results`;
* a default Evaluation is unchanged: no new key, a six-field EvalResult."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import path_metric_cases as PM                                      # noqa: E402
import r2r_world                                                    # noqa: E402
import r2r_val_seen as VS                                           # noqa: E402

LISTS = ('nav_errors', 'oracle_errors', 'trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success')
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
    from speaker_follower_amd import env
    items, gold = r2r_world.load()
    graphs = {s: env.NavGraph(os.path.join(r2r_world.CONN, s + '_connectivity.json')) for s in gold['config']['scans']}
    return items, gold, graphs


@pytest.fixture(scope='module')
def g10b():
    from speaker_follower_amd import env, nav_data
    items, _ = VS.load_items()
    gold = VS.load_sr_golden()
    scans = sorted({it['scan'] for it in items})
    conn = nav_data.connectivity_dir(scans=scans)
    graphs = {s: env.NavGraph(os.path.join(conn, s + '_connectivity.json')) for s in scans}
    return items, gold, graphs


@pytest.fixture(scope='module')
def synthetic():
    graphs, cases = PM.graphs(), PM.cases()
    ev, results = PM.evaluation_of(cases, graphs, path_metrics=True, device='cpu')
    want = [PM.restate(ev.table.block(s), P, R) for s, P, R in cases]
    return cases, ev, results, want


def test_known_answers_on_the_unit_line_graph():
    from speaker_follower_amd import evaluation
    cases = [('b_line6', P, R) for R, P, *_ in PM.KNOWN]
    ev, results = PM.evaluation_of(cases, PM.graphs(), path_metrics=True, device='cpu')
    D = ev.table.block('b_line6')
    assert [D[0][k] for k in range(6)] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    for i, (R, P, dtw, ndtw, success, spl, sdtw) in enumerate(PM.KNOWN):
        r = ev._score_item('%d_0' % i, results['%d_0' % i]['trajectory'])
        assert isinstance(r, evaluation.PathEvalResult) and r._fields == PM.FIELDS
        assert r.dtw == dtw and r.ndtw == ndtw, (i, r)
        assert PM.restate(D, P, R) == tuple(r)
        if success is not None:
            assert r.success is success and r.spl == spl
        if sdtw is not None:
            assert r.sdtw == sdtw
    second = ev._score_item('1_0', results['1_0']['trajectory'])
    assert second.nav_error == 3.0 and not second.success             # an error of exactly 3.0 is not a success
    first = ev._score_item('0_0', results['0_0']['trajectory'])
    assert first.sdtw == 1.0 and first.shortest_length == 3.0


@pytest.mark.parametrize('name', ['g10', 'g10b'])
def test_recorded_trajectories_equal_the_restatement_per_item(name, request):
    from speaker_follower_amd import evaluation
    items, gold, graphs = request.getfixturevalue(name)
    results = results_of(gold)
    assert len(results) == (156 if name == 'g10' else 782)
    ev = evaluation.Evaluation(items=items, graphs=graphs, path_metrics=True, device='cpu')
    plain = evaluation.Evaluation(items=items, graphs=graphs, device='cpu')
    summary, scores = ev.score_results(results)
    want_summary, want_scores = plain.score_results(results)
    for k in LISTS:
        assert list(scores[k]) == list(want_scores[k]), k            # (== on floats: to the last bit)
    for k in SUMMARY + ('model_score',):
        assert summary[k] == want_summary[k], k
    assert list(summary) == list(want_summary) + ['spl', 'ndtw', 'sdtw']
    t = ev.table
    scored = [k for k in results if k in ev.instr_ids]
    assert len(scored) == len(scores['dtw']) == len(ev.instr_ids)
    for i, k in enumerate(scored):
        gt = ev.gt[int(k.split('_')[0])]
        ix = t.index[gt['scan']]
        want = PM.restate(t.block(gt['scan']), [ix[p[0]] for p in results[k]['trajectory']], [ix[v] for v in gt['path']])
        got = tuple(scores[name][i] for name in LISTS + PM.PATH_LISTS)
        assert got == want, k
        assert tuple(ev._score_item(k, results[k]['trajectory'])) == want
    for k in ('spl', 'ndtw', 'sdtw'):
        assert summary[k] == np.average(scores[k])
        assert 0.0 <= summary[k] <= 1.0
    assert summary['sdtw'] <= summary['ndtw'] and summary['spl'] <= summary['success_rate']
    print('%s: spl %.4f ndtw %.4f sdtw %.4f at success_rate %.4f'
          % (name, summary['spl'], summary['ndtw'], summary['sdtw'], summary['success_rate']))


def test_gold_paths_scored_as_their_own_predictions(g10b):
    from speaker_follower_amd import evaluation
    items, gold, graphs = g10b
    ev = evaluation.Evaluation(items=items, graphs=graphs, path_metrics=True, device='cpu')
    assert len(ev.gt) == 260
    ids = ['%d_0' % p for p in ev.gt]
    got = ev.score_routes(ids, [[(v, 0.0, 0.0) for v in gt['path']] for gt in ev.gt.values()])
    assert len(got) == 260
    for r, gt in zip(got, ev.gt.values()):
        assert r.dtw == 0.0 and r.ndtw == 1.0 and r.spl == 1.0 and r.sdtw == 1.0, gt['path_id']
        assert r.trajectory_length == r.shortest_length and r.success


def test_the_cost_is_taken_from_the_pose_to_the_gold_node(synthetic):
    cases, ev, results, want = synthetic
    D = ev.table.block('c_order')
    assert D[0][3] != D[3][0]
    for P, R in (([0], [0, 3]), ([0, 1, 0], [0, 3])):
        i = cases.index(('c_order', P, R))
        r = ev._score_item('%d_0' % i, results['%d_0' % i]['trajectory'])
        assert r.dtw == PM.dtw_of(D, P, R)
        assert r.dtw != PM.dtw_of(D, P, R, transposed=True)
    i = cases.index(('c_order', [0], [0, 3]))
    assert want[i][7] == 0.0 + D[0][3] and want[i][7] != D[3][0]


def test_two_components_and_start_equals_goal(synthetic):
    cases, ev, results, want = synthetic
    for P, R in (([0, 1, 2], [0, 7, 8]), ([0, 7, 1], [0, 1, 2]), ([0, 1], [0, 1, 9])):
        i = cases.index(('d_two_parts', P, R))
        r = ev._score_item('%d_0' % i, results['%d_0' % i]['trajectory'])
        assert math.isinf(r.dtw) and r.ndtw == 0.0 and r.sdtw == 0.0
        assert not any(isinstance(v, float) and math.isnan(v) for v in r), r
        assert tuple(r) == want[i]
    unreachable = ev._score_item('%d_0' % i, results['%d_0' % i]['trajectory'])
    assert math.isinf(unreachable.shortest_length) and not unreachable.success and unreachable.spl == 0.0
    i = cases.index(('a_single', [0], [0]))
    r = ev._score_item('%d_0' % i, results['%d_0' % i]['trajectory'])
    assert r.success and r.trajectory_steps == 0 and r.spl == 1.0 and r.ndtw == 1.0 and r.sdtw == 1.0


def test_the_shared_cases_equal_the_restatement_on_every_entry(synthetic):
    cases, ev, results, want = synthetic
    assert len(cases) == PM.N_CASES and {len(R) for _, _, R in cases} >= {1, 2, 63, 64}
    assert {len(P) for _, P, _ in cases} >= {1, 2, 64, 65, 130}
    ids = list(results)
    one_by_one = [tuple(ev._score_item(k, results[k]['trajectory'])) for k in ids]
    assert one_by_one == want
    assert [tuple(r) for r in ev.score_routes(ids, [results[k]['trajectory'] for k in ids])] == want
    summary, scores = ev.score_results(results)
    for j, name in enumerate(LISTS + PM.PATH_LISTS):
        assert list(scores[name]) == [w[j] for w in want], name
    assert summary['ndtw'] == np.average([w[9] for w in want])
    assert any(math.isinf(w[7]) for w in want) and not any(math.isnan(v) for w in want for v in w)


def test_a_route_that_starts_elsewhere_is_refused(synthetic):
    cases, ev, results, want = synthetic
    with pytest.raises(AssertionError, match='should include the start position'):
        ev.score_routes(['0_0'], [[('v1', 0.0, 0.0)]])


def test_a_default_evaluation_is_unchanged(g10):
    from speaker_follower_amd import evaluation
    items, gold, graphs = g10
    results = results_of(gold)
    ev = evaluation.Evaluation(items=items, graphs=graphs, device='cpu')
    assert ev.path_metrics is False
    summary, scores = ev.score_results(results)
    assert set(summary) == set(SUMMARY) | {'model_score'} and set(scores) == set(LISTS)
    k = next(iter(results))
    r = ev._score_item(k, results[k]['trajectory'])
    assert type(r) is evaluation.EvalResult and len(r) == 6
    many = ev.score_routes(list(results), [results[i]['trajectory'] for i in results])
    assert all(type(x) is evaluation.EvalResult for x in many)
    assert many == [ev._score_item(i, results[i]['trajectory']) for i in results]


def test_the_bare_name_module_exports_the_new_names(monkeypatch):
    from speaker_follower_amd import compat, evaluation
    monkeypatch.syspath_prepend(compat.path())
    sys.modules.pop('eval', None)
    import eval as bare
    try:
        assert bare.PathEvalResult is evaluation.PathEvalResult and bare.path_metrics_of is evaluation.path_metrics_of
    finally:
        sys.modules.pop('eval', None)
