"""GPU: sf_eval_score_routes_coverage (csrc/sf_eval_routes.hip) alone, and CLS end to end -- against the plain-Python
restatement of tests/coverage_metric_cases.py, with == everywhere.

* the kernel through ctypes, `near` filled with a NaN pattern first: B = 1, 4, 5, 257, gold paths of 1, 2, 63, 64 nodes,
  routes of 1, 2, 8, 9, 64, 65, 130 poses (n + g on, under and over multiples of the prefetch depth and of the
  wavefront), a scan of one node, inf distances, unit-weight ties, slot -1; columns b >= g, the rows of unwritten slots
  and the words behind the array keep the pattern; the eight classic outputs == sf_eval_score_routes on the same arrays;
  the sweep layout == the ragged one; every per-route refusal, the new `g > near_ld` one among them; the SF_ERR_ARG and
  SF_ERR_UNSUPPORTED cases.
* Evaluation(coverage_metrics=True) with the table on the device: score_results == the device='cpu' evaluator with one
  host sync, score_routes == _score_item; a path_metrics and a default evaluator return what they returned.
* score_agent with the switch on == agent.test() + score_results, one host sync.
* run_rational_follower(compute_oracle=True): every candidate's eval_result == _score_item."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coverage_metric_cases as CM                                  # noqa: E402
import path_metric_cases as PM                                      # noqa: E402
import r2r_world                                                    # noqa: E402
import search_world as W                                            # noqa: E402

DEV = torch.device('cuda', 0)
SENTINEL, ISENTINEL, TAIL = -7.25, -9, 8
NAN_BITS = 0x7ff80badcafe0123                                       # a quiet NaN no computation produces
LISTS = ('nav_errors', 'oracle_errors', 'trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success')
SUMMARY = ('nav_error', 'oracle_error', 'steps', 'lengths', 'success_rate', 'oracle_rate')
ALL_LISTS = LISTS + PM.PATH_LISTS + CM.COVERAGE_LISTS


# ------------------------------------------------------------------------------------------ the kernel alone
@pytest.fixture(scope='module')
def world():
    """The shared cases, their host distance table (NavGraph.shortest), the restatement and `near` of every case, once."""
    from speaker_follower_amd import evaluation
    graphs, cases = PM.graphs(), CM.cases()
    t = evaluation.DistanceTable(graphs, device='cpu')
    base, n = {}, 100                                              # (nav rows of a larger table: scan bases are not 0)
    for s in t.scans:
        base[s], n = n, n + t.m[s]
    return dict(t=t, cases=cases, base=base, table=torch.from_numpy(t.host).to(DEV),
                want=[CM.restate(t.block(s), P, R) for s, P, R in cases],
                near=[CM.near_of(t.block(s), P, R) for s, P, R in cases])


def host_arrays(w, cases, slots, layout):
    """The host arrays of one launch over `cases` ([(scan, P, R)]; gold path k is case k's) in either layout."""
    t, base = w['t'], w['base']
    B = len(cases)
    a = dict(gold_off=np.cumsum([0] + [len(R) for _, _, R in cases]).astype(np.int32),
             gold_node=np.concatenate([R for _, _, R in cases]).astype(np.int32),
             gold_id=np.arange(B, dtype=np.int32),
             scan_base=np.array([base[s] for s, _, _ in cases], np.int32),
             m=np.array([t.m[s] for s, _, _ in cases], np.int32),
             dist_off=np.array([t.off[s] for s, _, _ in cases], np.int64),
             slot=np.asarray(slots, np.int32))
    n = [len(P) - 1 for _, P, _ in cases]
    if layout == 'ragged':
        a.update(S=0, row_stride=1, actions=None, n_steps=np.asarray(n, np.int32),
                 row=np.concatenate([np.asarray(P) + base[s] for s, P, _ in cases]).astype(np.int32),
                 row_first=np.cumsum([0] + [k + 1 for k in n[:-1]]).astype(np.int64))
    else:                                                          # what a rollout leaves behind: row [S+1,B], actions [S,B]
        S = max(n)
        assert min(n) >= 1
        row = np.array([[base[s] + P[min(k, len(P) - 1)] for s, P, _ in cases] for k in range(S + 1)], np.int32)
        act = np.ones((S, B), np.int64)
        for b, k in enumerate(n):
            if k < S:
                act[k - 1, b] = 0                                  # a stop ends it; k == S: the episode never stops
                act[k:, b] = np.arange(S - k) % 3                  # (whatever follows the first stop is not read)
        a.update(S=S, row_stride=B, actions=act, n_steps=None, row=row, row_first=np.arange(B, dtype=np.int64))
    a.update(B=B, n_gold=B, n_gold_nodes=len(a['gold_node']), max_gold=max(len(R) for _, _, R in cases),
             n_rows=a['row'].size)
    return a


def launch(w, a, n_slots, near_ld=None, null_near=False):
    """One launch over the host arrays `a`: sf_eval_score_routes_coverage with `near` [n_slots, near_ld] (+ TAIL words)
    when near_ld is given, else sf_eval_score_routes.  -> (status, float64 [5, n_slots + TAIL], int32 [3, ...], err,
    the int64 words of `near`)."""
    from speaker_follower_amd import _lib
    up = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in a.items() if isinstance(v, np.ndarray)}
    f64 = torch.full((5, n_slots + TAIL), SENTINEL, dtype=torch.float64, device=DEV)
    i32 = torch.full((3, n_slots + TAIL), ISENTINEL, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda k: up[k].data_ptr() if k in up else None                                   # noqa: E731
    e = _lib.EvalRoutes(a['S'], a['B'], n_slots, a['row_stride'], a['n_gold'], a['n_gold_nodes'], a['max_gold'], 0,
                        a['n_rows'], p('row'), p('row_first'), p('n_steps'), p('actions'), p('gold_off'), p('gold_node'),
                        p('gold_id'), p('scan_base'), p('m'), p('dist_off'), p('slot'), w['table'].data_ptr(), PM.MARGIN,
                        *[f64[k].data_ptr() for k in range(5)], *[i32[k].data_ptr() for k in range(3)])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    words = None
    if near_ld is None:
        status = _lib.lib.sf_eval_score_routes(C.byref(e), C.c_void_p(err.data_ptr()), st)
    else:
        words = torch.full((n_slots * max(near_ld, 1) + TAIL,), NAN_BITS, dtype=torch.int64, device=DEV)
        status = _lib.lib.sf_eval_score_routes_coverage(C.byref(e), None if null_near else C.c_void_p(words.data_ptr()),
                                                        near_ld, C.c_void_p(err.data_ptr()), st)
    torch.cuda.synchronize()
    return status, f64.cpu().numpy(), i32.cpu().numpy(), int(err.item()), None if words is None else words.cpu().numpy()


def eight(f64, i32, slot):
    """One slot in the order of CM.FIELDS[:8]."""
    return (f64[0, slot], f64[1, slot], i32[0, slot], f64[2, slot], bool(i32[1, slot]), bool(i32[2, slot]),
            f64[3, slot], f64[4, slot])


def check_slots(out, slots, n_slots, near_ld, cases, want, near, skip=()):
    """Every written slot == the restatement, its `near` row == near_of on the first g words; every other slot, every
    word of a row from g on, and the tail of every array, holds its sentinel."""
    _, f64, i32, _, words = out
    rows = words[:n_slots * near_ld].reshape(n_slots, near_ld)
    used = set()
    for b, slot in enumerate(slots):
        if slot < 0 or b in skip:
            continue
        used.add(slot)
        g = len(cases[b][2])
        assert i32[1, slot] in (0, 1) and i32[2, slot] in (0, 1)
        assert eight(f64, i32, slot) == want[b][:8], (b, eight(f64, i32, slot), want[b][:8])
        got = rows[slot, :g].view(np.float64).tolist()
        assert got == near[b] and got[0] == 0.0, (b, got, near[b])
        assert (rows[slot, :g] == np.asarray(near[b], np.float64).view(np.int64)).all()      # the same bits
        assert (rows[slot, g:] == NAN_BITS).all(), b
    rest = sorted(set(range(n_slots + TAIL)) - used)
    assert (f64[:, rest] == SENTINEL).all() and (i32[:, rest] == ISENTINEL).all()
    assert (rows[[s for s in range(n_slots) if s not in used]] == NAN_BITS).all()
    assert (words[n_slots * near_ld:] == NAN_BITS).all() and len(words) == n_slots * near_ld + TAIL


def same_eight(out, plain):
    assert out[0] == plain[0] and out[3] == plain[3]
    assert (out[1].view(np.int64) == plain[1].view(np.int64)).all() and (out[2] == plain[2]).all()


@pytest.mark.parametrize('B', [1, 4, 5, 257])
def test_coverage_kernel_equals_the_restatement_bit_for_bit(world, B):
    w = world
    block = next(i for i, (s, _, _) in enumerate(w['cases']) if s == 'e_rand70')          # GOLDS x POSES starts here
    first = {1: CM.first_of(w['cases'], 64, 65), 4: 0, 5: block, 257: 0}[B]
    cases, want, near = (w[k][first:first + B] for k in ('cases', 'want', 'near'))
    assert len(cases) == B
    rng = np.random.default_rng(B)
    n_slots = B + 3
    slots = [int(x) for x in rng.permutation(n_slots)[:B]]
    longest = max(len(R) for _, _, R in cases)
    near_ld = longest + (3 if B == 5 else 0)                       # (a row wider than the longest gold path)
    if B == 5:
        assert [(len(R), len(P)) for _, P, R in cases] == [(1, k) for k in CM.POSES[:5]]
    if B == 257:
        for b in (2, 40, 256):
            slots[b] = -1
        assert {(len(R), len(P)) for _, P, R in cases} >= {(g, k) for g in CM.GOLDS for k in CM.POSES}
        assert any(s == 'a_single' for s, _, _ in cases) and any(np.isinf(x[3]) for x in want)
        assert any(s in ('b_line6', 'f_grid9') for s, _, _ in cases) and near_ld == 64
    a = host_arrays(w, cases, slots, 'ragged')
    out = launch(w, a, n_slots, near_ld)
    assert out[0] == 0 and out[3] == 0
    check_slots(out, slots, n_slots, near_ld, cases, want, near)
    same_eight(out, launch(w, a, n_slots))                         # sf_eval_score_routes on the same arrays


def test_inf_distances(world):
    """Gold nodes no pose can reach: an inf in `near`, stored as such; a pose nobody can walk to: every `near` finite."""
    w = world
    cases = CM.UNREACHABLE + [('d_two_parts', [0, 7, 1], [0, 1, 2])]
    D = w['t'].block('d_two_parts')
    want = [CM.restate(D, P, R) for _, P, R in cases]
    near = [CM.near_of(D, P, R) for _, P, R in cases]
    assert all(np.inf in x for x in near[:3]) and np.inf not in near[3] and np.isinf(want[3][3])
    slots = [3, 1, 0, 2]
    a = host_arrays(w, cases, slots, 'ragged')
    out = launch(w, a, 4, 3)
    assert out[0] == 0 and out[3] == 0
    check_slots(out, slots, 4, 3, cases, want, near)
    same_eight(out, launch(w, a, 4))


def test_sweep_layout_equals_ragged_layout(world):
    w = world
    keep = [i for i, (_, P, _) in enumerate(w['cases']) if len(P) >= 2]
    cases, want, near = ([w[k][i] for i in keep] for k in ('cases', 'want', 'near'))
    B = len(cases)
    assert B > 130 and max(len(P) for _, P, _ in cases) == 130
    slots = list(range(B))
    slots[7] = -1
    ragged = launch(w, host_arrays(w, cases, slots, 'ragged'), B, 64)
    a = host_arrays(w, cases, slots, 'sweep')
    assert a['S'] == 129 and (a['actions'] != 0).all(0).any()      # (an episode that never stops is among them)
    sweep = launch(w, a, B, 64)
    assert ragged[0] == sweep[0] == 0 and ragged[3] == sweep[3] == 0
    same_eight(sweep, ragged)
    assert (ragged[4] == sweep[4]).all()                           # the same words, written and unwritten
    check_slots(sweep, slots, B, 64, cases, want, near)
    same_eight(sweep, launch(w, a, B))


def _longer_gold_than_the_row(a):
    a['max_gold'] = 3                                              # (a host copy that understates the table)


REFUSALS = {
    'slot_out_of_range': lambda a: a['slot'].__setitem__(2, 9),
    'slot_below_minus_one': lambda a: a['slot'].__setitem__(2, -2),
    'pose_outside_its_scan': lambda a: a['row'].__setitem__(int(a['row_first'][2]) + 1, int(a['scan_base'][2]) + int(a['m'][2])),
    'pose_below_its_scan': lambda a: a['row'].__setitem__(int(a['row_first'][2]) + 1, int(a['scan_base'][2]) - 1),
    'gold_node_outside_its_scan': lambda a: a['gold_node'].__setitem__(int(a['gold_off'][2]) + 1, int(a['m'][2])),
    'wrong_start': lambda a: a['row'].__setitem__(int(a['row_first'][2]), int(a['row'][int(a['row_first'][2]) + 1])),
    'gold_id_out_of_range': lambda a: a['gold_id'].__setitem__(2, 5),
    'gold_id_negative': lambda a: a['gold_id'].__setitem__(2, -1),
    'negative_step_count': lambda a: a['n_steps'].__setitem__(2, -1),
    'steps_beyond_the_row_array': lambda a: a['n_steps'].__setitem__(2, 10 ** 6),
    'row_first_beyond_the_row_array': lambda a: a['row_first'].__setitem__(2, 10 ** 9),
    'gold_path_longer_than_a_row_of_near': _longer_gold_than_the_row,
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_a_refused_route_writes_nothing_and_raises_err(world, name):
    w = world
    cases = [('e_rand70', [5, 9, 11], [5, 6]), ('b_line6', [0, 1], [0, 1, 2]), ('e_rand70', [3, 7, 8, 9], [3, 4, 5, 6]),
             ('f_grid9', [0, 1, 2], [0, 2]), ('b_line6', [4], [4, 5])]
    want = [CM.restate(w['t'].block(s), P, R) for s, P, R in cases]
    near = [CM.near_of(w['t'].block(s), P, R) for s, P, R in cases]
    slots = [4, 3, 2, 1, 0]
    a = host_arrays(w, cases, slots, 'ragged')
    assert a['max_gold'] == 4
    REFUSALS[name](a)
    near_ld = a['max_gold']                                        # (4; 3 where the host copy understates: route 2 has 4)
    out = launch(w, a, 5, near_ld)
    assert out[0] == 0 and out[3] == 1
    check_slots(out, [4, 3, -1, 1, 0], 5, near_ld, cases, want, near)       # route 2 wrote nothing, the others are scored


def test_a_gold_path_of_no_nodes_and_one_above_the_limit_are_refused_by_the_kernel(world):
    w = world
    cases = [('b_line6', [0, 1], [0, 1, 2]), ('e_rand70', [3] * 3, [3] + list(range(64))), ('b_line6', [4], [4, 5])]
    want = [CM.restate(w['t'].block(s), P, R) for s, P, R in cases]
    near = [CM.near_of(w['t'].block(s), P, R) for s, P, R in cases]
    a = host_arrays(w, cases, [0, 1, 2], 'ragged')
    assert a['max_gold'] == 65
    a['max_gold'] = 64                                             # (a host copy that understates the table)
    out = launch(w, a, 3, 66)                                      # (rows wide enough: the limit refuses, not the row)
    assert out[0] == 0 and out[3] == 1
    check_slots(out, [0, -1, 2], 3, 66, cases, want, near)
    a = host_arrays(w, cases[:1] + cases[2:], [0, 1], 'ragged')
    a['gold_off'][:] = [0, 3, 3]                                   # gold path 1 is empty
    out = launch(w, a, 2, 3)
    assert out[0] == 0 and out[3] == 1
    check_slots(out, [0, -1], 2, 3, cases, want, near)


def test_refusals_of_the_entry(world):
    from speaker_follower_amd import _lib
    w = world
    lib = _lib.lib
    cases, want, near = (w[k][:5] for k in ('cases', 'want', 'near'))
    slots = list(range(5))
    longest = max(len(R) for _, _, R in cases)
    nothing = lambda out, ld: check_slots(out, [-1] * 5, 5, ld, cases, None, None)       # noqa: E731
    # a gold path above the limit in the host copy: SF_ERR_UNSUPPORTED, nothing launched
    a = host_arrays(w, cases, slots, 'ragged')
    a['max_gold'] = 65
    out = launch(w, a, 5, 65)
    assert out[0] == _lib.SF_ERR_UNSUPPORTED and out[3] == 0
    nothing(out, 65)
    # SF_ERR_ARG: a row of near shorter than the longest gold path, no near at all
    a['max_gold'] = longest
    out = launch(w, a, 5, longest - 1)
    assert out[0] == _lib.SF_ERR_ARG and out[3] == 0
    nothing(out, longest - 1)
    out = launch(w, a, 5, longest, null_near=True)
    assert out[0] == _lib.SF_ERR_ARG and out[3] == 0
    nothing(out, longest)
    out = launch(w, a, 5, longest)
    assert out[0] == 0 and out[3] == 0
    check_slots(out, slots, 5, longest, cases, want, near)
    # NULL pointers and sizes below 1, as sf_eval_score_routes refuses them
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    one = torch.zeros(16, dtype=torch.float64, device=DEV)
    p = one.data_ptr()
    assert lib.sf_eval_score_routes_coverage(None, C.c_void_p(p), 1, C.c_void_p(p), st) == _lib.SF_ERR_ARG
    ok = {f: (p if ty is C.c_void_p else 1) for f, ty in _lib.EvalRoutes._fields_}
    ok.update(margin=3.0, reserved=0)
    pointers = [f for f, ty in _lib.EvalRoutes._fields_ if ty is C.c_void_p and f not in ('n_steps', 'actions')]
    assert len(pointers) == 18
    bad_cases = ([{f: None} for f in pointers] +
                 [{f: v} for f in ('B', 'n_slots', 'row_stride', 'n_gold', 'n_gold_nodes', 'max_gold', 'n_rows')
                  for v in (0, -1)] +
                 [dict(n_steps=None, actions=None), dict(n_steps=None, S=0), dict(n_steps=None, S=-1)])
    for bad in bad_cases:
        e = _lib.EvalRoutes(**dict(ok, **bad))
        assert lib.sf_eval_score_routes_coverage(C.byref(e), C.c_void_p(p), 1, C.c_void_p(p), st) == _lib.SF_ERR_ARG, bad
    e = _lib.EvalRoutes(**ok)
    assert lib.sf_eval_score_routes_coverage(C.byref(e), C.c_void_p(p), 1, None, st) == _lib.SF_ERR_ARG
    assert lib.sf_eval_score_routes_coverage(C.byref(e), None, 1, C.c_void_p(p), st) == _lib.SF_ERR_ARG
    assert lib.sf_eval_score_routes_coverage(C.byref(e), C.c_void_p(p), 0, C.c_void_p(p), st) == _lib.SF_ERR_ARG
    torch.cuda.synchronize()
    assert (one == 0).all()
    assert lib.sf_abi_version() == 10


# ------------------------------------------------------------------------------------------ Evaluation on the device
def results_of(gold):
    out = {}
    for k, v in gold['items'].items():
        el = v.get('elevations', [0.0] * len(v['viewpoints']))
        out[k] = dict(instr_id=k, trajectory=[(a, h, e) for a, h, e in zip(v['viewpoints'], v['headings'], el)],
                      score=v['score'])
    return out


def make_agent(env, store, weights, episode_len):
    from speaker_follower_amd import agents, model, synth
    d = synth.FULL
    enc_w, dec_w = weights
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    enc.cuda().eval()
    dec.cuda().eval()
    state = random.getstate()
    agent = agents.Seq2SeqAgent(env, '/tmp/sf_coverage_metrics.json', enc, dec, episode_len=episode_len)
    random.setstate(state)
    agent.store = store
    return agent


@pytest.fixture(scope='module')
def g10_world():
    from speaker_follower_amd import evaluation, features, nav, synth
    items, gold = r2r_world.load()
    cfg = gold['config']
    env, table, graphs = r2r_world.build_env(items, cfg, dense=False)
    store = features.FeatureStore(table)
    agent = make_agent(env, store, synth.follower_weights_peaky(cfg['weight_seed']), cfg['episode_len'])
    agent.use_device_env(nav.NavTable(env, store))
    return dict(gold=gold, env=env, agent=agent, graphs=graphs, items=items,
                ev=evaluation.Evaluation(env=env, coverage_metrics=True),
                path=evaluation.Evaluation(env=env, path_metrics=True), plain=evaluation.Evaluation(env=env))


def test_score_results_on_the_device_equals_the_host_evaluator(g10_world):
    from speaker_follower_amd import evaluation
    w = g10_world
    results = results_of(w['gold'])
    ev = w['ev']
    host = evaluation.Evaluation(items=w['items'], graphs=w['graphs'], coverage_metrics=True, device='cpu')
    assert ev.table.dev is not None and host.table.dev is None
    syncs, fallbacks = ev.host_syncs, ev.fallbacks
    summary, scores = ev.score_results(results)
    assert ev.host_syncs == syncs + 1 and ev.last_host_syncs == 1 and ev.fallbacks == fallbacks
    want_summary, want_scores = host.score_results(results)
    assert host.host_syncs == 0
    assert set(scores) == set(ALL_LISTS) and len(scores['cls']) == 156
    for k in ALL_LISTS:
        assert list(scores[k]) == list(want_scores[k]), k          # (== on floats: to the last bit)
    assert summary == want_summary and list(summary) == list(want_summary)
    assert list(summary)[-4:] == ['spl', 'ndtw', 'sdtw', 'cls']
    # a path_metrics evaluator and a default one: what they returned before, equal to the leading part of the above
    for kind, lists, last in (('path', LISTS + PM.PATH_LISTS, 'sdtw'), ('plain', LISTS, 'model_score')):
        other = w[kind]
        other_host = evaluation.Evaluation(items=w['items'], graphs=w['graphs'], path_metrics=kind == 'path', device='cpu')
        s, sc = other.score_results(results)
        hs, hsc = other_host.score_results(results)
        assert other.coverage_metrics is False and set(sc) == set(lists) and list(s)[-1] == last and 'cls' not in s
        assert s == hs and {k: list(v) for k, v in sc.items()} == {k: list(v) for k, v in hsc.items()}
        for k in lists:
            assert list(sc[k]) == list(scores[k]), k
        for k in s:
            assert s[k] == summary[k], k


def test_score_routes_equals_score_item(g10_world):
    from speaker_follower_amd import evaluation
    w = g10_world
    results = results_of(w['gold'])
    ids = [k for k in results if k in w['ev'].instr_ids]
    paths = [results[k]['trajectory'] for k in ids]
    for ev, kind in ((w['ev'], evaluation.CoverageEvalResult), (w['path'], evaluation.PathEvalResult),
                     (w['plain'], evaluation.EvalResult)):
        syncs = ev.host_syncs
        got = ev.score_routes(ids, paths)
        assert ev.host_syncs == syncs + 1                          # one launch, one sync for the batch
        want = [ev._score_item(k, p) for k, p in zip(ids, paths)]
        assert all(type(r) is kind for r in got) and all(type(r) is kind for r in want)
        assert [tuple(r) for r in got] == [tuple(r) for r in want]
        assert [r._asdict() for r in got] == [r._asdict() for r in want]
    with pytest.raises(AssertionError, match='should include the start position'):
        goal = w['ev'].gt[int(ids[0].split('_')[0])]['path'][-1]
        w['ev'].score_routes(ids[:1], [[(goal, 0.0, 0.0)] + paths[0]])


class Rewind:
    """The environment's item order and `random` as they were: two walks from the same state."""

    def __init__(self, env):
        self.env, self.data, self.state = env, list(env.data), random.getstate()

    def __call__(self):
        self.env.data[:] = self.data
        random.setstate(self.state)


def test_score_agent_with_the_switch_on(g10_world):
    w = g10_world
    agent, ev, path, plain = w['agent'], w['ev'], w['path'], w['plain']
    rewind = Rewind(w['env'])
    results = agent.test(use_dropout=False, feedback='argmax')
    assert all(hasattr(r, 'nav_rows') for r in results.values())   # results of a device rollout: scored from their rows
    want_summary, want_scores = ev.score_results(results)
    want_scores = {k: list(v) for k, v in want_scores.items()}
    assert ev.last_host_syncs == 1
    losses = list(agent.losses)
    rewind()
    fallbacks, sweeps = ev.fallbacks, ev.sweeps
    summary, scores = ev.score_agent(agent)
    assert ev.fallbacks == fallbacks and ev.sweeps == sweeps + 1 and ev.last_host_syncs == 1
    assert set(scores) == set(ALL_LISTS)
    for k in ALL_LISTS:
        assert list(scores[k]) == want_scores[k], k
    assert summary == want_summary and set(summary) == set(SUMMARY) | {'model_score', 'spl', 'ndtw', 'sdtw', 'cls'}
    assert agent.losses == losses
    print('g10: cls %.4f beside ndtw %.4f sdtw %.4f at success_rate %.4f'
          % (summary['cls'], summary['ndtw'], summary['sdtw'], summary['success_rate']))
    # a path_metrics evaluator and a default one: their lists and keys, as before, equal to the leading part of the above
    for other, lists, keys in ((path, LISTS + PM.PATH_LISTS, {'model_score', 'spl', 'ndtw', 'sdtw'}),
                               (plain, LISTS, {'model_score'})):
        rewind()
        other_summary, other_scores = other.score_agent(agent)
        assert other.last_host_syncs == 1 and set(other_scores) == set(lists)
        assert set(other_summary) == set(SUMMARY) | keys
        for k in lists:
            assert list(other_scores[k]) == want_scores[k], k
        for k in other_summary:
            assert other_summary[k] == want_summary[k], k
    rewind()


# ------------------------------------------------------------------------------------------ run_rational_follower
@pytest.fixture(scope='module')
def search_world():
    from speaker_follower_amd import model, features, agents, synth
    env, table = W.build_world(dense=True)
    d = synth.FULL
    enc_w, dec_w = synth.follower_weights(W.FOLLOWER_SEED)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    enc.cuda().eval()
    dec.cuda().eval()
    agent = agents.Seq2SeqAgent(env, '/tmp/sf_coverage_metrics_search.json', enc, dec, episode_len=W.EPISODE_LEN)
    agent.store = features.FeatureStore(table)
    senc_w, sdec_w = synth.speaker_weights(W.SPEAKER_SEED)
    senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    senc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    sdec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    senc.cuda().eval()
    sdec.cuda().eval()
    speaker = agents.Seq2SeqSpeaker(env, '/tmp/sf_coverage_metrics_spk.json', senc, sdec, W.INSTRUCTION_LEN,
                                    max_episode_len=W.EPISODE_LEN)
    return env, agent, speaker


class PerCandidate:
    """An evaluator without `score_routes`: run_rational_follower then scores candidate by candidate."""

    def __init__(self, ev):
        self._score_item, self.score_results = ev._score_item, ev.score_results


def test_rational_follower_candidates_carry_the_new_fields(search_world, monkeypatch):
    from speaker_follower_amd import evaluation, search
    env, agent, speaker = search_world
    ev = evaluation.Evaluation(env=env, coverage_metrics=True)
    ev.instr_ids = {it['instr_id'] for it in env.data}            # (the world holds one instruction per path)
    assert ev.table.dev is not None
    seen = []
    mix = search.rational_mix
    monkeypatch.setattr(search, 'rational_mix', lambda by, wt: seen.append(by) or mix(by, wt))
    calls = []
    batch = ev.score_routes
    monkeypatch.setattr(ev, 'score_routes', lambda ids, paths: calls.append(len(ids)) or batch(ids, paths))
    rewind = Rewind(env)                                           # (the item order and `random`: the same walk twice)
    how = dict(state_factored_search=True, physical_traversal=True)                       # (the long routes)
    got, picks = search.run_rational_follower(env, ev, agent, speaker, beam_size=3, compute_oracle=True, **how)
    fallbacks = ev.fallbacks
    n, cls = 0, set()
    for group in seen[0].values():
        for c in group:
            assert c['eval_result'] == ev._score_item(c['instr_id'], c['trajectory'])._asdict()
            assert tuple(c['eval_result']) == evaluation.CoverageEvalResult._fields
            cls.add(c['eval_result']['cls'])
            n += 1
    assert n > W.N_ITEMS and sum(calls) >= n and len(calls) <= W.N_ITEMS // W.BATCH + 1   # one batch per minibatch
    assert fallbacks == 0 and len(cls) > 1 and all(0.0 <= x <= 1.0 for x in cls)
    rewind()
    want, want_picks = search.run_rational_follower(env, PerCandidate(ev), agent, speaker, beam_size=3,
                                                    compute_oracle=True, **how)
    assert got == want and picks == want_picks and set(got) == {0.0, 0.95}
    assert list(seen[0]) == list(seen[2])
    for k, group in seen[0].items():
        assert [c['eval_result'] for c in group] == [c['eval_result'] for c in seen[2][k]], k
    assert 'cls' in got[0.0] and 'spl' in got[0.0]
    rewind()
