"""CPU: CLS (coverage weighted by length score) of `evaluation.Evaluation(coverage_metrics=True)` against its definition
restated in tests/coverage_metric_cases.py, with == everywhere.

* the hand-checked rows on the unit line graph;
* the direction of `near` (D[pose][gold node]); two components: an inf in `near`, a gold path of infinite length;
* per item over the recorded trajectories of the g10 and g10b goldens (156 and 782 results); the classic six and the
  five path fields against an Evaluation(path_metrics=True); a default and a path_metrics evaluator are unchanged;
* the 260 val-seen gold paths as their own predictions: coverage, length_score and cls 1.0;
* the shared case list through `_score_item`, `score_routes` and `score_results`;
* the result type, the score lists, the summary key, the bare-name module's exports;
* the header: ABI 10, the new symbol exported and bound, sf_eval_routes as it was."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coverage_metric_cases as CM                                  # noqa: E402
import path_metric_cases as PM                                      # noqa: E402
import r2r_world                                                    # noqa: E402
import r2r_val_seen as VS                                           # noqa: E402

LISTS = ('nav_errors', 'oracle_errors', 'trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success')
SUMMARY = ('nav_error', 'oracle_error', 'steps', 'lengths', 'success_rate', 'oracle_rate')
ALL_LISTS = LISTS + PM.PATH_LISTS + CM.COVERAGE_LISTS


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
    graphs, cases = PM.graphs(), CM.cases()
    ev, results = PM.evaluation_of(cases, graphs, coverage_metrics=True, device='cpu')
    want = [CM.restate(ev.table.block(s), P, R) for s, P, R in cases]
    return cases, ev, results, want


def score_one(scan_cases, i=0, **kw):
    ev, results = PM.evaluation_of(scan_cases, PM.graphs(), device='cpu', **kw)
    return ev, ev._score_item('%d_0' % i, results['%d_0' % i]['trajectory'])


def test_hand_checked_rows_on_the_unit_line_graph():
    from speaker_follower_amd import evaluation
    cases = [('b_line6', P, R) for R, P, *_ in CM.KNOWN]
    ev, results = PM.evaluation_of(cases, PM.graphs(), coverage_metrics=True, device='cpu')
    assert ev.coverage_metrics is True and ev.path_metrics is True
    D = ev.table.block('b_line6')
    assert [D[0][k] for k in range(6)] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    for i, (R, P, coverage, length_score, cls) in enumerate(CM.KNOWN):
        r = ev._score_item('%d_0' % i, results['%d_0' % i]['trajectory'])
        assert type(r) is evaluation.CoverageEvalResult and r._fields == CM.FIELDS
        assert (r.coverage, r.length_score, r.cls) == (coverage, length_score, cls), (i, r)
        assert r.gold_length == float(len(R) - 1)
        assert tuple(r) == CM.restate(D, P, R)
    c = (1.0 + math.exp(-1.0 / 3.0) + math.exp(-2.0 / 3.0) + math.exp(-1.0)) / 4
    second = ev._score_item('1_0', results['1_0']['trajectory'])
    assert second.coverage == c and second.cls == c / 2 and second.trajectory_length == 0


def test_near_is_taken_from_the_pose_to_the_gold_node(monkeypatch):
    from speaker_follower_amd import evaluation
    P, R = [0], [0, 3]
    seen = []
    formed = evaluation.coverage_metrics_of
    monkeypatch.setattr(evaluation, 'coverage_metrics_of', lambda r, near, *a: seen.append(list(near)) or formed(r, near, *a))
    ev, r = score_one([('c_order', P, R)], coverage_metrics=True)
    D = ev.table.block('c_order')
    assert D[0][3] == (0.1 + 0.2) + 0.3 and D[3][0] == (0.3 + 0.2) + 0.1 and D[0][3] != D[3][0]
    assert seen == [[0.0, float(D[0][3])]] == [CM.near_of(D, P, R)]
    assert seen[0] != CM.near_of(D, P, R, transposed=True) == [0.0, float(D[3][0])]
    assert all(type(x) is float for x in seen[0])
    assert r.coverage == (1.0 + math.exp(-D[0][3] / 3.0)) / 2 == CM.coverage_of(CM.near_of(D, P, R))
    assert tuple(r) == CM.restate(D, P, R)
    assert r.gold_length == D[0][3] and r.gold_length != D[3][0]     # the gold length walks the gold path's way too


def test_two_components():
    for i, (s, P, R) in enumerate(CM.UNREACHABLE):
        ev, r = score_one(CM.UNREACHABLE, i, coverage_metrics=True)
        D = ev.table.block(s)
        near = CM.near_of(D, P, R)
        assert near[0] == 0.0 and math.inf in near                    # a gold node no pose can reach
        assert math.isinf(r.gold_length) and r.length_score == 0.0 and r.cls == 0.0
        assert 1.0 / len(R) <= r.coverage < 1.0
        assert not any(isinstance(v, float) and math.isnan(v) for v in r), r
        assert tuple(r) == CM.restate(D, P, R)
    # a POSE nobody can walk to: every gold node is still reached, the route is infinitely long
    case = ('d_two_parts', [0, 7, 1], [0, 1, 2])
    ev, r = score_one([case], coverage_metrics=True)
    assert math.isinf(r.trajectory_length) and math.isfinite(r.gold_length) and r.coverage > 0
    assert r.length_score == 0.0 and r.cls == 0.0
    assert not any(isinstance(v, float) and math.isnan(v) for v in r), r


def test_coverage_metrics_of_on_its_corner_values():
    from speaker_follower_amd import evaluation
    inf = math.inf
    base = evaluation.PathEvalResult(0.0, 0.0, 0, 0.0, True, True, 0.0, 0.0, 1.0, 1.0, 1.0)
    f = evaluation.coverage_metrics_of
    assert f(base, [0.0], 0.0, 3.0)[11:] == (0.0, 1.0, 1.0, 1.0)                   # stays put on a one-node gold path
    assert f(base._replace(trajectory_length=2.0), [0.0], 0.0, 3.0)[11:] == (0.0, 1.0, 0.0, 0.0)
    assert f(base._replace(trajectory_length=inf), [0.0, 1.0], 1.0, 3.0)[13:] == (0.0, 0.0)
    got = f(base._replace(trajectory_length=inf), [0.0, inf], inf, 3.0)           # no inf - inf, no inf / inf
    assert got[11:] == (inf, 0.5, 0.0, 0.0)
    assert f(base, [0.0, inf, inf], 4.0, 3.0).coverage == 1.0 / 3.0
    for near, length, gold_length in (([0.0, 0.5, 2.5], 3.25, 2.75), ([0.0, 7.0], 0.0, 7.0)):
        want = CM.four_of(near, gold_length, length)
        assert f(base._replace(trajectory_length=length), near, gold_length, 3.0)[11:] == want


@pytest.mark.parametrize('name', ['g10', 'g10b'])
def test_recorded_trajectories_equal_the_restatement_per_item(name, request):
    from speaker_follower_amd import evaluation
    items, gold, graphs = request.getfixturevalue(name)
    results = results_of(gold)
    assert len(results) == (156 if name == 'g10' else 782)
    ev = evaluation.Evaluation(items=items, graphs=graphs, coverage_metrics=True, device='cpu')
    path = evaluation.Evaluation(items=items, graphs=graphs, path_metrics=True, device='cpu')
    plain = evaluation.Evaluation(items=items, graphs=graphs, device='cpu')
    assert (path.path_metrics, path.coverage_metrics, plain.path_metrics, plain.coverage_metrics) == \
        (True, False, False, False)
    summary, scores = ev.score_results(results)
    path_summary, path_scores = path.score_results(results)
    plain_summary, plain_scores = plain.score_results(results)
    # the two earlier evaluators: their present types, lists and summaries
    assert set(plain_scores) == set(LISTS) and set(path_scores) == set(LISTS + PM.PATH_LISTS)
    assert list(plain_summary) == list(SUMMARY) + ['model_score']
    assert list(path_summary) == list(plain_summary) + ['spl', 'ndtw', 'sdtw']
    k0 = next(iter(results))
    assert type(plain._score_item(k0, results[k0]['trajectory'])) is evaluation.EvalResult
    assert type(path._score_item(k0, results[k0]['trajectory'])) is evaluation.PathEvalResult
    # the new one: the earlier lists and keys with the same bits, then its own
    assert set(scores) == set(ALL_LISTS) and list(summary) == list(path_summary) + ['cls']
    for k in LISTS + PM.PATH_LISTS:
        assert list(scores[k]) == list(path_scores[k]), k            # (== on floats: to the last bit)
    for k in path_summary:
        assert summary[k] == path_summary[k], k
    t = ev.table
    scored = [k for k in results if k in ev.instr_ids]
    assert len(scored) == len(scores['cls']) == len(ev.instr_ids)
    for i, k in enumerate(scored):
        gt = ev.gt[int(k.split('_')[0])]
        ix = t.index[gt['scan']]
        want = CM.restate(t.block(gt['scan']), [ix[p[0]] for p in results[k]['trajectory']], [ix[v] for v in gt['path']])
        assert tuple(scores[n][i] for n in ALL_LISTS) == want, k
        r = ev._score_item(k, results[k]['trajectory'])
        assert type(r) is evaluation.CoverageEvalResult and tuple(r) == want
        assert tuple(r)[:11] == tuple(path._score_item(k, results[k]['trajectory']))
    assert summary['cls'] == np.average(scores['cls']) and 0.0 < summary['cls'] <= 1.0
    assert all(0.0 < c <= 1.0 for c in scores['coverage']) and all(0.0 <= s <= 1.0 for s in scores['length_score'])
    print('%s: cls %.4f beside ndtw %.4f sdtw %.4f at success_rate %.4f'
          % (name, summary['cls'], summary['ndtw'], summary['sdtw'], summary['success_rate']))


def test_gold_paths_scored_as_their_own_predictions(g10b):
    from speaker_follower_amd import evaluation
    items, gold, graphs = g10b
    ev = evaluation.Evaluation(items=items, graphs=graphs, coverage_metrics=True, device='cpu')
    assert len(ev.gt) == 260
    ids = ['%d_0' % p for p in ev.gt]
    got = ev.score_routes(ids, [[(v, 0.0, 0.0) for v in gt['path']] for gt in ev.gt.values()])
    assert len(got) == 260
    for r, gt in zip(got, ev.gt.values()):
        assert r.coverage == 1.0 and r.length_score == 1.0 and r.cls == 1.0, gt['path_id']
        assert r.gold_length == r.trajectory_length and r.ndtw == 1.0


def test_the_shared_cases_equal_the_restatement_on_every_entry(synthetic):
    cases, ev, results, want = synthetic
    assert len(cases) == CM.N_CASES
    assert {(len(R), len(P)) for _, P, R in cases} >= {(g, k) for g in CM.GOLDS for k in CM.POSES}
    ids = list(results)
    one_by_one = [tuple(ev._score_item(k, results[k]['trajectory'])) for k in ids]
    assert one_by_one == want
    assert [tuple(r) for r in ev.score_routes(ids, [results[k]['trajectory'] for k in ids])] == want
    summary, scores = ev.score_results(results)
    for j, name in enumerate(ALL_LISTS):
        assert list(scores[name]) == [w[j] for w in want], name
    assert summary['cls'] == np.average([w[14] for w in want])
    assert not any(math.isinf(w[11]) for w in want)                   # every gold path inside one component
    assert any(math.isinf(w[3]) for w in want) and not any(math.isnan(v) for w in want for v in w)
    assert len({w[14] for w in want}) > 100 and any(w[14] == 1.0 for w in want) and any(w[14] == 0.0 for w in want)
    assert ev.fallbacks == 0 and ev.host_syncs == 0


def test_result_type_lists_and_exports(monkeypatch):
    from speaker_follower_amd import compat, evaluation
    R = evaluation.CoverageEvalResult
    assert R._fields == evaluation.PathEvalResult._fields + ('gold_length', 'coverage', 'length_score', 'cls')
    assert R._fields[:6] == evaluation.EvalResult._fields and len(R._fields) == 15
    ev, r = score_one([('b_line6', [0, 1], [0, 1, 2])], coverage_metrics=True)
    assert type(r) is R and list(r._asdict()) == list(CM.FIELDS)
    many = ev.score_routes(['0_0'], [[('v0', 0.0, 0.0), ('v1', 0.0, 0.0)]])
    assert [type(x) for x in many] == [R] and many == [r]
    assert type(score_one([('b_line6', [0, 1], [0, 1, 2])], path_metrics=True)[1]) is evaluation.PathEvalResult
    assert type(score_one([('b_line6', [0, 1], [0, 1, 2])])[1]) is evaluation.EvalResult
    both = evaluation.Evaluation(items=[], graphs={}, path_metrics=False, coverage_metrics=True, device='cpu')
    assert both.path_metrics is True and both.coverage_metrics is True
    monkeypatch.syspath_prepend(compat.path())
    sys.modules.pop('eval', None)
    import eval as bare
    try:
        assert bare.CoverageEvalResult is R and bare.coverage_metrics_of is evaluation.coverage_metrics_of
        assert bare.PathEvalResult is evaluation.PathEvalResult and bare.Evaluation is evaluation.Evaluation
    finally:
        sys.modules.pop('eval', None)


def test_header_and_abi():
    from speaker_follower_amd import _lib
    assert _lib.lib.sf_abi_version() == 10 == _lib.ABI_VERSION
    name = 'sf_eval_score_routes_coverage'
    assert name in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), name)
    decl = _lib.HEADER.functions[name]
    assert decl.ret == ('int', 0)
    assert decl.params == [('e', 'sf_eval_routes', 1), ('near', 'double', 1), ('near_ld', 'int32_t', 0),
                           ('err', 'int32_t', 1), ('stream', 'sf_stream', 0)]
    fn = getattr(_lib.lib, name)
    assert fn.argtypes == [C.POINTER(_lib.EvalRoutes), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int
    assert _lib.HEADER.functions['sf_eval_score_routes'].params == [('e', 'sf_eval_routes', 1), ('err', 'int32_t', 1),
                                                                    ('stream', 'sf_stream', 0)]
    # sf_eval_routes as it was: the same members at the same places
    assert [n for n, _ in _lib.EvalRoutes._fields_] == [
        'S', 'B', 'n_slots', 'row_stride', 'n_gold', 'n_gold_nodes', 'max_gold', 'reserved', 'n_rows', 'row', 'row_first',
        'n_steps', 'actions', 'gold_off', 'gold_node', 'gold_id', 'scan_base', 'm', 'dist_off', 'slot', 'table', 'margin',
        'nav_error', 'oracle_error', 'length', 'shortest', 'dtw', 'steps', 'success', 'oracle_success']
    assert C.sizeof(_lib.EvalRoutes) == 8 * 4 + 8 + 12 * 8 + 8 + 8 * 8
    assert (_lib.EvalRoutes.n_rows.offset, _lib.EvalRoutes.margin.offset, _lib.EvalRoutes.steps.offset) == (32, 136, 184)
    assert _lib.SF_EVAL_MAX_GOLD == 64
    # refused before anything touches the device
    assert fn(None, None, 0, None, None) == _lib.SF_ERR_ARG
