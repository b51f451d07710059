"""GPU: sf_eval_score_routes (csrc/sf_eval_routes.hip) alone, and the path-fidelity metrics end to end -- against the
plain-Python restatement of tests/path_metric_cases.py, with ==.

* the kernel through ctypes, sentinels behind every output array: B = 1, 4, 5, 257 (routes per workgroup, the grid
  edge), gold paths of 1, 2, 63, 64 nodes, routes of 1, 2, 64, 65, 130 poses (more anti-diagonals than lanes), a scan of
  one node, inf distances, ties among all three predecessors, slot -1; the sweep layout against the ragged one and its
  classic six against sf_eval_score on the same arrays; S = 1; every refusal; the SF_ERR_ARG / SF_ERR_UNSUPPORTED cases.
* Evaluation(path_metrics=True) with the table on the device: score_results == the device='cpu' evaluator with one host
  sync, score_routes == _score_item for both result types.
* score_agent with the metrics on == agent.test() + score_results, one host sync; a default evaluator is unchanged.
* run_rational_follower(compute_oracle=True): every candidate's eval_result == _score_item, the summaries == those of
  the per-candidate loop."""
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
import path_metric_cases as PM                                      # noqa: E402
import r2r_world                                                    # noqa: E402
import search_world as W                                            # noqa: E402

DEV = torch.device('cuda', 0)
SENTINEL, ISENTINEL, TAIL = -7.25, -9, 8
LISTS = ('nav_errors', 'oracle_errors', 'trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success')
SUMMARY = ('nav_error', 'oracle_error', 'steps', 'lengths', 'success_rate', 'oracle_rate')


# ------------------------------------------------------------------------------------------ the kernel alone
@pytest.fixture(scope='module')
def world():
    """The shared cases, their host distance table (NavGraph.shortest) and the restatement of every case, computed once."""
    from speaker_follower_amd import evaluation
    graphs, cases = PM.graphs(), PM.cases()
    t = evaluation.DistanceTable(graphs, device='cpu')
    want = [PM.restate(t.block(s), P, R) for s, P, R in cases]
    base, n = {}, 100                                              # (nav rows of a larger table: scan bases are not 0)
    for s in t.scans:
        base[s], n = n, n + t.m[s]
    return dict(t=t, cases=cases, want=want, base=base, table=torch.from_numpy(t.host).to(DEV))


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


def launch(w, a, n_slots):
    """sf_eval_score_routes over the host arrays `a`: (status, float64 [5, n_slots + TAIL], int32 [3, ...], err)."""
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
    status = _lib.lib.sf_eval_score_routes(C.byref(e), C.c_void_p(err.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status, f64.cpu().numpy(), i32.cpu().numpy(), int(err.item())


def eight(f64, i32, slot):
    """One slot in the order of PM.FIELDS[:8]."""
    return (f64[0, slot], f64[1, slot], i32[0, slot], f64[2, slot], bool(i32[1, slot]), bool(i32[2, slot]),
            f64[3, slot], f64[4, slot])


def check_slots(f64, i32, slots, n_slots, want, skip=()):
    """Every written slot == the restatement; every other one, and the tail of every array, holds its sentinel."""
    used = set()
    for b, slot in enumerate(slots):
        if slot < 0 or b in skip:
            continue
        used.add(slot)
        assert i32[1, slot] in (0, 1) and i32[2, slot] in (0, 1)
        assert eight(f64, i32, slot) == want[b][:8], (b, eight(f64, i32, slot), want[b][:8])
    rest = sorted(set(range(n_slots + TAIL)) - used)
    assert (f64[:, rest] == SENTINEL).all() and (i32[:, rest] == ISENTINEL).all()


@pytest.mark.parametrize('B', [1, 4, 5, 257])
def test_routes_kernel_equals_the_restatement_bit_for_bit(world, B):
    w = world
    first = {1: 33, 4: 0, 5: 15, 257: 0}[B]                       # (B = 5: gold paths of 1 node, routes of 1 .. 130 poses;
    cases, want = w['cases'][first:first + B], w['want'][first:first + B]     # B = 1: 64 gold nodes, 65 poses)
    assert len(cases) == B
    rng = np.random.default_rng(B)
    n_slots = B + 3
    slots = [int(x) for x in rng.permutation(n_slots)[:B]]
    if B == 257:
        for b in (2, 40, 256):
            slots[b] = -1
        assert {len(R) for _, _, R in cases} >= {1, 2, 63, 64} and {len(P) for _, P, _ in cases} >= {1, 2, 64, 65, 130}
        assert any(np.isinf(x[7]) for x in want) and any(s == 'a_single' for s, _, _ in cases)
    status, f64, i32, err = launch(w, host_arrays(w, cases, slots, 'ragged'), n_slots)
    assert status == 0 and err == 0
    check_slots(f64, i32, slots, n_slots, want)


def test_sweep_layout_equals_ragged_layout_and_sf_eval_score(world):
    from speaker_follower_amd import _lib
    w = world
    keep = [i for i, (_, P, _) in enumerate(w['cases']) if len(P) >= 2]
    cases, want = [w['cases'][i] for i in keep], [w['want'][i] for i in keep]
    B = len(cases)
    assert B > 130 and max(len(P) for _, P, _ in cases) == 130
    slots = list(range(B))
    slots[7] = -1
    ragged = launch(w, host_arrays(w, cases, slots, 'ragged'), B)
    a = host_arrays(w, cases, slots, 'sweep')
    assert a['S'] == 129 and (a['actions'] != 0).all(0).any()      # (an episode that never stops is among them)
    sweep = launch(w, a, B)
    assert ragged[0] == sweep[0] == 0 and ragged[3] == sweep[3] == 0
    assert (ragged[1] == sweep[1]).all() and (ragged[2] == sweep[2]).all()             # the same bits (inf == inf)
    check_slots(sweep[1], sweep[2], slots, B, want)
    # the classic six of sf_eval_score on the same sweep-layout arrays
    up = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in a.items() if isinstance(v, np.ndarray)}
    goal = torch.from_numpy(np.array([w['base'][s] + R[-1] for s, _, R in cases], np.int32)).to(DEV)
    f64 = torch.full((3, B), SENTINEL, dtype=torch.float64, device=DEV)
    i32 = torch.full((3, B), ISENTINEL, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda k: up[k].data_ptr()                                                        # noqa: E731
    ep = _lib.EvalEpisodes(a['S'], B, B, 0, p('row'), p('actions'), goal.data_ptr(), p('scan_base'), p('m'), p('dist_off'),
                           p('slot'), w['table'].data_ptr(), PM.MARGIN, *[f64[k].data_ptr() for k in range(3)],
                           *[i32[k].data_ptr() for k in range(3)])
    _lib.call('sf_eval_score', C.byref(ep), C.c_void_p(err.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    assert (f64.cpu().numpy() == sweep[1][:3, :B]).all() and (i32.cpu().numpy() == sweep[2][:, :B]).all()


def test_sweep_layout_at_one_step(world):
    """S = 1: a stop at step 0 and an episode that never stops are both one step long."""
    w = world
    cases = [('b_line6', [2, 3], [2, 3, 4]), ('f_grid9', [4, 4], [4, 5])]
    want = [PM.restate(w['t'].block(s), P, R) for s, P, R in cases]
    a = host_arrays(w, cases, [1, 0], 'sweep')
    assert a['S'] == 1
    a['actions'][0] = [0, 2]
    status, f64, i32, err = launch(w, a, 2)
    assert status == 0 and err == 0
    check_slots(f64, i32, [1, 0], 2, want)
    assert i32[0, 0] == 1 and i32[0, 1] == 1


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
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_a_refused_route_writes_nothing_and_raises_err(world, name):
    w = world
    cases = [('e_rand70', [5, 9, 11], [5, 6]), ('b_line6', [0, 1], [0, 1, 2]), ('e_rand70', [3, 7, 8, 9], [3, 4, 5]),
             ('f_grid9', [0, 1, 2], [0, 2]), ('b_line6', [4], [4, 5])]
    want = [PM.restate(w['t'].block(s), P, R) for s, P, R in cases]
    slots = [4, 3, 2, 1, 0]
    a = host_arrays(w, cases, slots, 'ragged')
    REFUSALS[name](a)
    status, f64, i32, err = launch(w, a, 5)
    assert status == 0 and err == 1
    check_slots(f64, i32, [4, 3, -1, 1, 0], 5, want)              # route 2 wrote nothing, the others are scored


def test_a_gold_path_of_no_nodes_and_one_above_the_limit_are_refused_by_the_kernel(world):
    w = world
    cases = [('b_line6', [0, 1], [0, 1, 2]), ('e_rand70', [3] * 3, [3] + list(range(64))), ('b_line6', [4], [4, 5])]
    want = [PM.restate(w['t'].block(s), P, R) for s, P, R in cases]
    a = host_arrays(w, cases, [0, 1, 2], 'ragged')
    assert a['max_gold'] == 65
    a['max_gold'] = 64                                             # (a host copy that understates the table)
    status, f64, i32, err = launch(w, a, 3)
    assert status == 0 and err == 1
    check_slots(f64, i32, [0, -1, 2], 3, want)
    a = host_arrays(w, cases[:1] + cases[2:], [0, 1], 'ragged')
    a['gold_off'][:] = [0, 3, 3]                                   # gold path 1 is empty
    status, f64, i32, err = launch(w, a, 2)
    assert status == 0 and err == 1
    check_slots(f64, i32, [0, -1], 2, want)


def test_refusals_of_the_entry(world):
    from speaker_follower_amd import _lib
    w = world
    lib = _lib.lib
    cases = w['cases'][:5]
    slots = list(range(5))
    # a gold path above the limit in the host copy: nothing launched
    a = host_arrays(w, cases, slots, 'ragged')
    a['max_gold'] = 65
    status, f64, i32, err = launch(w, a, 5)
    assert status == _lib.SF_ERR_UNSUPPORTED and err == 0
    check_slots(f64, i32, [-1] * 5, 5, None)
    a['max_gold'] = 64
    assert launch(w, a, 5)[0] == 0
    # NULL pointers and sizes below 1
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sf_eval_score_routes(None, None, st) == _lib.SF_ERR_ARG
    one = torch.zeros(16, dtype=torch.float64, device=DEV)
    p = one.data_ptr()
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
        assert lib.sf_eval_score_routes(C.byref(e), C.c_void_p(p), st) == _lib.SF_ERR_ARG, bad
    assert lib.sf_eval_score_routes(C.byref(_lib.EvalRoutes(**ok)), None, st) == _lib.SF_ERR_ARG
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
    agent = agents.Seq2SeqAgent(env, '/tmp/sf_path_metrics.json', enc, dec, episode_len=episode_len)
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
                ev=evaluation.Evaluation(env=env, path_metrics=True), plain=evaluation.Evaluation(env=env))


def test_score_results_on_the_device_equals_the_host_evaluator(g10_world):
    from speaker_follower_amd import evaluation
    w = g10_world
    results = results_of(w['gold'])
    ev = w['ev']
    host = evaluation.Evaluation(items=w['items'], graphs=w['graphs'], path_metrics=True, device='cpu')
    assert ev.table.dev is not None and host.table.dev is None
    syncs, fallbacks = ev.host_syncs, ev.fallbacks
    summary, scores = ev.score_results(results)
    assert ev.host_syncs == syncs + 1 and ev.last_host_syncs == 1 and ev.fallbacks == fallbacks
    want_summary, want_scores = host.score_results(results)
    assert host.host_syncs == 0
    assert set(scores) == set(LISTS + PM.PATH_LISTS) and len(scores['dtw']) == 156
    for k in LISTS + PM.PATH_LISTS:
        assert list(scores[k]) == list(want_scores[k]), k          # (== on floats: to the last bit)
    assert summary == want_summary and list(summary) == list(want_summary)
    assert list(summary)[-3:] == ['spl', 'ndtw', 'sdtw']


def test_score_routes_equals_score_item_for_both_result_types(g10_world):
    from speaker_follower_amd import evaluation
    w = g10_world
    results = results_of(w['gold'])
    ids = [k for k in results if k in w['ev'].instr_ids]
    paths = [results[k]['trajectory'] for k in ids]
    for ev, kind in ((w['ev'], evaluation.PathEvalResult), (w['plain'], evaluation.EvalResult)):
        syncs = ev.host_syncs
        got = ev.score_routes(ids, paths)
        assert ev.host_syncs == syncs + 1                          # one launch, one sync for the batch
        assert all(type(r) is kind for r in got)
        want = [ev._score_item(k, p) for k, p in zip(ids, paths)]
        assert all(type(r) is kind for r in want)
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


def test_score_agent_with_the_metrics_on(g10_world):
    w = g10_world
    agent, ev, plain = w['agent'], w['ev'], w['plain']
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
    assert set(scores) == set(LISTS + PM.PATH_LISTS)
    for k in LISTS + PM.PATH_LISTS:
        assert list(scores[k]) == want_scores[k], k
    assert summary == want_summary and set(summary) == set(SUMMARY) | {'model_score', 'spl', 'ndtw', 'sdtw'}
    assert agent.losses == losses
    print('g10: spl %.4f ndtw %.4f sdtw %.4f at success_rate %.4f'
          % (summary['spl'], summary['ndtw'], summary['sdtw'], summary['success_rate']))
    # a default evaluator: the six lists and keys, as before, and equal to the classic part of the above
    rewind()
    plain_summary, plain_scores = plain.score_agent(agent)
    assert plain.last_host_syncs == 1 and set(plain_scores) == set(LISTS)
    assert set(plain_summary) == set(SUMMARY) | {'model_score'}
    for k in LISTS:
        assert list(plain_scores[k]) == want_scores[k], k
    for k in plain_summary:
        assert plain_summary[k] == want_summary[k], k
    rewind()
    by_test, by_test_scores = plain.score_results(agent.test(use_dropout=False, feedback='argmax'))
    assert by_test == plain_summary and {k: list(v) for k, v in by_test_scores.items()} == dict(plain_scores)
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
    agent = agents.Seq2SeqAgent(env, '/tmp/sf_path_metrics_search.json', enc, dec, episode_len=W.EPISODE_LEN)
    agent.store = features.FeatureStore(table)
    senc_w, sdec_w = synth.speaker_weights(W.SPEAKER_SEED)
    senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    senc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    sdec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    senc.cuda().eval()
    sdec.cuda().eval()
    speaker = agents.Seq2SeqSpeaker(env, '/tmp/sf_path_metrics_spk.json', senc, sdec, W.INSTRUCTION_LEN,
                                    max_episode_len=W.EPISODE_LEN)
    return env, agent, speaker


class PerCandidate:
    """An evaluator without `score_routes`: run_rational_follower then scores candidate by candidate, as it did before
    the batch entry existed."""

    def __init__(self, ev):
        self._score_item, self.score_results = ev._score_item, ev.score_results


@pytest.mark.parametrize('path_metrics', [False, True])
def test_rational_follower_scores_its_candidates_in_one_batch(search_world, monkeypatch, path_metrics):
    from speaker_follower_amd import evaluation, search
    env, agent, speaker = search_world
    ev = evaluation.Evaluation(env=env, path_metrics=path_metrics)
    ev.instr_ids = {it['instr_id'] for it in env.data}            # (the world holds one instruction per path)
    assert ev.table.dev is not None
    seen = []
    mix = search.rational_mix
    monkeypatch.setattr(search, 'rational_mix', lambda by, wt: seen.append(by) or mix(by, wt))
    calls = []
    batch = ev.score_routes
    monkeypatch.setattr(ev, 'score_routes', lambda ids, paths: calls.append(len(ids)) or batch(ids, paths))
    rewind = Rewind(env)                                           # (the item order and `random`: the same walk twice)
    how = dict(state_factored_search=True, physical_traversal=True) if path_metrics else {}   # (the long routes / beams)
    got, picks = search.run_rational_follower(env, ev, agent, speaker, beam_size=3, compute_oracle=True, **how)
    fields = (evaluation.PathEvalResult if path_metrics else evaluation.EvalResult)._fields
    n = 0
    for group in seen[0].values():
        for c in group:
            assert c['eval_result'] == ev._score_item(c['instr_id'], c['trajectory'])._asdict()
            assert tuple(c['eval_result']) == fields
            n += 1
    assert n > W.N_ITEMS and sum(calls) >= n and len(calls) <= W.N_ITEMS // W.BATCH + 1   # one batch per minibatch
    rewind()
    want, want_picks = search.run_rational_follower(env, PerCandidate(ev), agent, speaker, beam_size=3,
                                                    compute_oracle=True, **how)
    assert got == want and picks == want_picks and set(got) == {0.0, 0.95}
    assert list(seen[0]) == list(seen[2])
    for k, group in seen[0].items():
        assert [c['eval_result'] for c in group] == [c['eval_result'] for c in seen[2][k]], k
    assert ('spl' in got[0.0]) == path_metrics
    rewind()
