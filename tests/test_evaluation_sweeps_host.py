"""CPU: the three pieces every evaluator sweep goes through.

* `sweeps.epoch_minibatches` against `BaseAgent.test` over the val-seen environment (782 instructions) at batch sizes
  1, 391 (divides the split), 100 (the epoch wraps inside a minibatch; sorted by length, fresh ids then lie behind a
  repeated one) and 1000 (larger than the split), with reset() and with reset(sort=True): the order of the first
  occurrences, `env.ix` and the state of `random` afterwards, with ==; `sweeps.snapshot` / `sweeps.restore`;
* `Evaluation._launch_route_scoring` with nothing launched: the struct the library would be handed, read back by field
  name in the three layouts (ragged, rollout sweep, walk sweep), every pointer the address it was given, the entry by
  `coverage_metrics`, the sentence of a raised err word per layout;
* `Evaluation._assemble` (the results, and with lists=True the `scores` lists) against `_score_item` over the recorded
  g10 / g10b trajectories and the shared synthetic cases (an unreachable goal, a gold path of one node), from o64 / o32
  / near built on the host.  The slots of a launch are handed out consecutively, so the empty ones lie behind the last
  ground truth, and behind a gold path's last node in its `near` row: both hold NaN / -1 here and must not be read."""
import ctypes as C
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coverage_metric_cases as CM                                  # noqa: E402
import path_metric_cases as PM                                      # noqa: E402
import r2r_world                                                    # noqa: E402
import r2r_val_seen as VS                                           # noqa: E402

SWITCHES = (dict(), dict(path_metrics=True), dict(coverage_metrics=True))


# ---------------------------------------------------------------------------------------------- epoch_minibatches
@pytest.fixture(scope='module')
def val_seen_env():
    items, _ = VS.load_items()
    env, _, _ = VS.build_env(items, batch_size=100)
    return env, list(env.data)


def walker(env, sort):
    """BaseAgent.test over a rollout that returns the minibatch's items."""
    from speaker_follower_amd import agents

    class Walker(agents.BaseAgent):
        def rollout(self):
            self.env.reset(sort=True) if sort else self.env.reset()
            return [dict(instr_id=it['instr_id']) for it in self.env.batch]
    return Walker(env, '')


@pytest.mark.parametrize('sort', [False, True])
@pytest.mark.parametrize('size', [1, 391, 100, 1000])
def test_epoch_minibatches_walks_what_base_agent_test_walks(val_seen_env, size, sort):
    from speaker_follower_amd import sweeps
    env, data0 = val_seen_env
    env.batch_size = size
    agent = walker(env, sort)                                         # (BaseAgent seeds `random`)
    state0 = random.getstate()
    env.data[:] = data0
    want = list(agent.test())
    want_ix, want_state = env.ix, random.getstate()
    assert len(want) == 782
    env.data[:] = data0
    random.setstate(state0)
    snap = sweeps.snapshot(env)
    env.reset_epoch()
    got, batches, last = [], [], None
    for k, items, fresh in sweeps.epoch_minibatches(env, sort=sort):
        assert k == len(batches) and items == env.batch and len(fresh) == len(items) == size
        assert last is None or all(last)                              # only the last minibatch holds a repeated id
        if sort:
            lengths = [len(it['instr_encoding']) for it in items]
            assert lengths == sorted(lengths, reverse=True)
        got += [it['instr_id'] for it, f in zip(items, fresh) if f]
        batches.append(items)
        last = fresh
    assert not all(last)
    assert got == want and env.ix == want_ix and random.getstate() == want_state
    assert len(batches) == -(-782 // size) + (782 % size == 0)
    if size == 100:                                                   # the epoch wraps inside the last minibatch:
        assert sum(last) == 82 and len(set(got)) == 782               # 82 fresh ids, 18 from the reshuffled front --
        assert any(last[last.index(False):]) == sort                  # sorted by length, fresh ones behind a repeated one
    if size == 1000:                                                  # an id twice in ONE minibatch: fresh only once
        assert len(batches) == 1 and sum(last) == 782
    assert env.data != data0 or size == 1                             # (the wrap shuffled the items ...)
    sweeps.restore(env, snap)                                         # ... and restore puts the walk's start back
    assert env.data == data0 and random.getstate() == state0
    env.batch_size = 100


def test_the_sweep_module_needs_neither_torch_nor_the_library():
    import subprocess
    code = ('import sys; import speaker_follower_amd.sweeps as s; '
            'assert "torch" not in sys.modules and "speaker_follower_amd._lib" not in sys.modules; '
            'assert s.epoch_minibatches and s.snapshot and s.restore')
    subprocess.run([sys.executable, '-c', code], check=True, cwd=os.path.dirname(HERE))


# ------------------------------------------------------------------------------------------ the launch helper's struct
class FakeLibrary:
    """Stands where _lib.lib stands: records the entry and its arguments, launches nothing."""

    def __init__(self, status=0):
        self.status, self.calls = status, []

    def __getattr__(self, name):
        if not name.startswith('sf_'):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or self.status


@pytest.fixture
def no_launch(monkeypatch):
    from speaker_follower_amd import _lib, runtime
    real = _lib.lib
    fake = FakeLibrary()
    fake.sf_status_string, fake.sf_last_error_string = real.sf_status_string, real.sf_last_error_string
    monkeypatch.setattr(_lib, 'lib', fake)
    monkeypatch.setattr(runtime, 'stream', lambda: C.c_void_p(0x5ea))
    return fake


def evaluator_with_tables(**kw):
    """An evaluator over the synthetic cases whose distance and gold tables 'are on a device': host tensors."""
    cases = CM.cases()[:12]
    ev, _ = PM.evaluation_of(cases, PM.graphs(), device='cpu', **kw)
    ev.table.dev = torch.from_numpy(ev.table.host)
    gold = ev._gold_table()
    gold['dev'] = tuple(torch.from_numpy(gold[k]) for k in ('off', 'node'))
    return ev, gold


def block(n, ld):
    return types.SimpleNamespace(o64=torch.zeros(5, n, dtype=torch.float64), o32=torch.zeros(3, n, dtype=torch.int32),
                                 err=torch.zeros(1, dtype=torch.int32), near=torch.zeros(n, ld, dtype=torch.float64))


LAYOUTS = {  # name -> (noun, S, B, n_slots, row_stride, n_steps given, actions given, the err word's sentence)
    'ragged': ('route', 0, 7, 7, 1, True, False, 'a route left its scan or does not start where its gold path does'),
    'rollout': ('rollout', 4, 5, 9, 5, False, True, 'a rollout left its scan, or a slot its array'),
    'walk': ('walk', 6, 5, 9, 5, True, True, 'a walk left its scan, or a slot its array')}
POINTERS = ('row', 'row_first', 'n_steps', 'actions', 'gold_id', 'scan_base', 'm', 'dist_off', 'slot')


@pytest.mark.parametrize('coverage', [False, True])
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_the_launch_helper_fills_the_struct_by_name(no_launch, layout, coverage):
    from speaker_follower_amd import _lib
    noun, S, B, n_slots, stride, with_steps, with_actions, sentence = LAYOUTS[layout]
    ev, gold = evaluator_with_tables(coverage_metrics=coverage, path_metrics=True)
    out = block(n_slots, gold['longest'])
    n_rows = 23 if layout == 'ragged' else (S + 1) * B
    i32, i64 = (lambda n: torch.zeros(n, dtype=torch.int32)), (lambda n: torch.zeros(n, dtype=torch.int64))
    given = dict(row=i32(n_rows), row_first=torch.arange(B, dtype=torch.int64), n_steps=i32(B) if with_steps else None,
                 actions=i64(max(S, 1) * B) if with_actions else None, gold_id=i32(B), scan_base=i32(B), m=i32(B),
                 dist_off=i64(B), slot=i32(B))
    assert len({t.data_ptr() for t in given.values() if t is not None}) == 7 + with_steps + with_actions
    status, text = ev._launch_route_scoring(out, noun, S=S, B=B, n_slots=n_slots, row_stride=stride, n_rows=n_rows,
                                            **given)
    assert status == 0 and len(no_launch.calls) == 1
    entry, args = no_launch.calls[0]
    assert entry == ('sf_eval_score_routes_coverage' if coverage else 'sf_eval_score_routes')
    e = args[0]._obj
    assert type(e) is _lib.EvalRoutes
    assert (e.S, e.B, e.n_slots, e.row_stride, e.n_rows, e.reserved) == (S, B, n_slots, stride, n_rows, 0)
    assert (e.n_gold, e.n_gold_nodes, e.max_gold) == (len(gold['ids']), len(gold['node']), gold['longest'])
    assert e.max_gold == max(len(R) for _, _, R in CM.cases()[:12]) and e.margin == 3.0
    for name in POINTERS:
        assert getattr(e, name) == (None if given[name] is None else given[name].data_ptr()), name
    if layout == 'ragged':
        assert e.row_stride == 1 and e.S == 0 and e.n_steps is not None and e.actions is None
    if layout == 'rollout':
        assert e.row_stride == B and e.n_steps is None and e.actions is not None
        first = (C.c_int64 * B).from_address(e.row_first)
        assert list(first) == list(range(B))
    if layout == 'walk':
        assert e.row_stride == B and e.n_steps is not None
    assert (e.gold_off, e.gold_node, e.table) == (gold['dev'][0].data_ptr(), gold['dev'][1].data_ptr(),
                                                  ev.table.dev.data_ptr())
    for k, name in enumerate(('nav_error', 'oracle_error', 'length', 'shortest', 'dtw')):
        assert getattr(e, name) == out.o64[k].data_ptr() == out.o64.data_ptr() + 8 * n_slots * k, name
    for k, name in enumerate(('steps', 'success', 'oracle_success')):
        assert getattr(e, name) == out.o32[k].data_ptr() == out.o32.data_ptr() + 4 * n_slots * k, name
    # behind the struct: (near, near_ld,) err, stream
    if coverage:
        assert len(args) == 5 and (args[1].value, args[2]) == (out.near.data_ptr(), gold['longest'])
    else:
        assert len(args) == 3
    assert args[-2].value == out.err.data_ptr() and args[-1].value == 0x5ea
    assert text == '%s: %s' % (entry, sentence)


def test_the_launch_helper_returns_a_refusal_and_raises_every_other_failure(no_launch):
    from speaker_follower_amd import _lib
    ev, gold = evaluator_with_tables(path_metrics=True)
    z = torch.zeros(8, dtype=torch.int64)
    args = dict(S=0, B=1, n_slots=1, row_stride=1, n_rows=1, row=z, row_first=z, n_steps=z, gold_id=z, scan_base=z, m=z,
                dist_off=z, slot=z)
    no_launch.status = _lib.SF_ERR_UNSUPPORTED
    assert ev._launch_route_scoring(block(1, 1), 'route', refusable=True, **args)[0] == _lib.SF_ERR_UNSUPPORTED
    for status, kw in ((_lib.SF_ERR_UNSUPPORTED, {}), (_lib.SF_ERR_ARG, {}), (_lib.SF_ERR_ARG, dict(refusable=True))):
        no_launch.status = status
        with pytest.raises(_lib.SfError, match='sf_eval_score_routes failed'):
            ev._launch_route_scoring(block(1, 1), 'route', **kw, **args)


def test_the_struct_and_its_entries_are_named_in_one_place():
    import glob
    import io
    import tokenize
    pkg = os.path.join(os.path.dirname(HERE), 'speaker_follower_amd')
    fills, named = 0, []
    for path in sorted(glob.glob(os.path.join(pkg, '*.py'))):
        text = open(path).read()
        fills += text.count('EvalRoutes(')
        for tok in tokenize.generate_tokens(io.StringIO(text).readline):
            if tok.type == tokenize.STRING and tok.string.strip('\'"') in ('sf_eval_score_routes',
                                                                           'sf_eval_score_routes_coverage'):
                named.append((os.path.basename(path), tok.string.strip('\'"')))
    assert fills == 1
    assert sorted(named) == [('evaluation.py', 'sf_eval_score_routes'), ('evaluation.py', 'sf_eval_score_routes_coverage')]


# ---------------------------------------------------------------------------------------------------- the assembler
def recorded(name):
    """(items, graphs, results) of a golden's recorded trajectories."""
    from speaker_follower_amd import env, nav_data
    if name == 'g10':
        items, gold = r2r_world.load()
        conn, scans = r2r_world.CONN, gold['config']['scans']
    else:
        items, _ = VS.load_items()
        gold = VS.load_sr_golden()
        scans = sorted({it['scan'] for it in items})
        conn = nav_data.connectivity_dir(scans=scans)
    graphs = {s: env.NavGraph(os.path.join(conn, s + '_connectivity.json')) for s in scans}
    results = {}
    for k, w in gold['items'].items():
        el = w.get('elevations', [0.0] * len(w['viewpoints']))
        results[k] = dict(instr_id=k, trajectory=[(v, h, e) for v, h, e in zip(w['viewpoints'], w['headings'], el)])
    return items, graphs, results


def synthetic():
    cases = CM.cases() + CM.UNREACHABLE
    assert any(len(R) == 1 for _, _, R in cases)
    items = [dict(path_id=i, scan=s, path=['v%d' % r for r in R]) for i, (s, _, R) in enumerate(cases)]
    results = {'%d_0' % i: dict(instr_id='%d_0' % i, trajectory=[('v%d' % p, 0.0, 0.0) for p in P])
               for i, (_, P, _) in enumerate(cases)}
    return items, PM.graphs(), results


@pytest.fixture(scope='module', params=['g10', 'g10b', 'synthetic'])
def world(request):
    return request.param, (synthetic() if request.param == 'synthetic' else recorded(request.param))


def outputs_on_the_host(ev, routes, empty):
    """What the scoring launch leaves for `routes` [(ground truth, local poses)] in slots 0 .. len(routes) - 1 of
    `empty` more: o64 [5, n], o32 [3, n], near [n, longest] from _score_six, D[start, goal], dtw_rows and the column
    minima.  What no route writes is NaN / -1."""
    from speaker_follower_amd import evaluation
    n = len(routes) + empty
    ld = max(len(gt['path']) for gt in ev.gt.values())
    o64, o32, near = np.full((5, n), np.nan), np.full((3, n), -1, np.int32), np.full((n, ld), np.nan)
    for i, (gt, rows) in enumerate(routes):
        scan, ix = gt['scan'], ev.table.index[gt['scan']]
        D, gold = ev.table.block(scan), [ix[v] for v in gt['path']]
        six = ev._score_six(scan, rows, gold[-1])
        cost = D[np.ix_(rows, gold)].tolist()
        o64[:, i] = six.nav_error, six.oracle_error, six.trajectory_length, D[rows[0], gold[-1]], evaluation.dtw_rows(cost)
        o32[:, i] = six.trajectory_steps, six.success, six.oracle_success
        near[i, :len(gold)] = [min(col) for col in zip(*cost)]
    return o64, o32, near


@pytest.mark.parametrize('switches', SWITCHES, ids=['plain', 'path', 'coverage'])
def test_the_assembler_equals_score_item_to_the_last_bit(world, switches):
    from speaker_follower_amd import evaluation
    name, (items, graphs, results) = world
    ev = evaluation.Evaluation(items=items, graphs=graphs, device='cpu', **switches)
    if name == 'synthetic':
        ev.instr_ids = set(results)
    ids = [k for k in results if k in ev.instr_ids]
    assert len(ids) == {'g10': 156, 'g10b': 780, 'synthetic': CM.N_CASES + 3}[name]
    want = [ev._score_item(k, results[k]['trajectory']) for k in ids]
    routes = [ev._route_of(k, results[k]['trajectory']) for k in ids]
    o64, o32, near = outputs_on_the_host(ev, routes, empty=5)
    if name == 'synthetic':
        assert np.isinf(o64[3, :len(ids)]).any() and np.isinf(near[:len(ids)]).any()    # an unreachable goal / gold node
    gts, near = [gt for gt, _ in routes], near if ev.coverage_metrics else None
    got = ev._assemble(gts, o64, o32, near)
    kind = (evaluation.CoverageEvalResult if ev.coverage_metrics else
            evaluation.PathEvalResult if ev.path_metrics else evaluation.EvalResult)
    assert len(got) == len(want) and all(type(r) is kind for r in got)
    for k, a, b in zip(ids, got, want):
        assert tuple(a) == tuple(b), k                                # (== on floats: to the last bit)
        assert (type(a.success), type(a.oracle_success), type(a.trajectory_steps)) == (bool, bool, int), k
    # the lists: the ones score_results leaves for the same results
    ev.scores = None
    scores = ev._assemble(gts, o64, o32, near, lists=True)
    assert scores is ev.scores
    lists = {n: list(v) for n, v in scores.items()}
    summary, want_scores = ev.score_results({k: results[k] for k in ids})
    assert set(lists) == set(want_scores) == {n for n, f in FIELD_OF.items() if f in kind._fields}
    for n in lists:
        assert lists[n] == list(want_scores[n]) == [getattr(r, FIELD_OF[n]) for r in want], n
    assert scores['missing'] == [] and type(scores['nav_errors']) is list


FIELD_OF = dict(nav_errors='nav_error', oracle_errors='oracle_error', trajectory_steps='trajectory_steps',
                trajectory_lengths='trajectory_length', success='success', oracle_success='oracle_success',
                shortest_lengths='shortest_length', dtw='dtw', spl='spl', ndtw='ndtw', sdtw='sdtw',
                gold_lengths='gold_length', coverage='coverage', length_score='length_score', cls='cls')


def test_no_results_leave_empty_lists():
    from speaker_follower_amd import evaluation
    ev = evaluation.Evaluation(items=[], graphs={}, coverage_metrics=True, device='cpu')
    ev.scores = None
    empty = [], np.zeros((5, 3)), np.zeros((3, 3), np.int32), np.zeros((3, 1))
    assert ev._assemble(*empty) == [] and ev.scores is None
    assert dict(ev._assemble(*empty, lists=True)) == {} and ev.scores['cls'] == []
