"""GPU: the evaluation kernels (csrc/sf_eval.hip) alone, and `Evaluation.score_agent` end to end.

* sf_eval_distances on synthetic graphs given as CSR, all in one launch, bit for bit against a host Dijkstra that
  accumulates d + w outward from the source (env.NavGraph.shortest): single node, a one-way edge, 63 / 64 / 65 nodes
  (lane ownership), a 70-node chain (more rounds than lanes), two components (inf blocks), weights whose sums depend on
  the direction of travel; then on real geometry: the largest R2R scan (348 viewpoints) and the five committed scans.
* sf_eval_score on a small synthetic world, per item bit for bit against oracle.np_env.score_results: a stop at step 0
  of S = 1, an episode that never stops, B = 1 and B = 65, slot -1, an oracle tie, an unreachable goal, an error of
  exactly 3.0 and of the largest double below it.
* score_agent == agent.test() + score_results(agent.results) in one process, on the g10 world and on val-seen at batch
  100: per-item arrays, summary, losses, env.ix and `random` afterwards; one host sync; no 'trajectory'; keep_results;
  the three fall-backs.
* the refusals of the C ABI and the host fill of a scan above the LDS limit (forced with the debug limit)."""
import ctypes as C
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import r2r_world                                                    # noqa: E402
import r2r_val_seen as VS                                           # noqa: E402
from oracle import np_env                                           # noqa: E402

DEV = torch.device('cuda', 0)
SENTINEL = -7.25
LISTS = ('nav_errors', 'oracle_errors', 'trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success')
SUMMARY = ('nav_error', 'oracle_error', 'steps', 'lengths', 'success_rate', 'oracle_rate')


# ------------------------------------------------------------------------------------------ synthetic graphs
def graph_of(n, edges):
    """An env.NavGraph over nodes 'v0' .. 'v<n-1>' (all included) with the DIRECTED weighted `edges` (u, v, w)."""
    from speaker_follower_amd.env import NavGraph
    g = NavGraph.__new__(NavGraph)
    g.ids = ['v%d' % i for i in range(n)]
    g.included = [True] * n
    g.adj, g._sp = {}, {}
    for u, v, w in edges:
        g.adj.setdefault(g.ids[u], {})[g.ids[v]] = float(w)
    return g


def both_ways(edges):
    return [e for u, v, w in edges for e in ((u, v, w), (v, u, w))]


def random_sparse(n, rng, extra):
    """A random spanning tree plus `extra` edges, symmetric irrational weights."""
    edges = [(i, int(rng.integers(i)), float(rng.uniform(0.3, 4.0))) for i in range(1, n)]
    for _ in range(extra):
        u, v = (int(x) for x in rng.integers(n, size=2))
        if u != v:
            edges.append((u, v, float(rng.uniform(0.3, 4.0))))
    return both_ways(edges)


def synthetic_graphs():
    rng = np.random.default_rng(5)
    g = {'a_single': graph_of(1, []),
         'b_one_way': graph_of(2, [(0, 1, 1.5)]),
         'f_chain70': graph_of(70, both_ways([(i, i + 1, 0.1 + 0.01 * i) for i in range(69)])),
         'g_two_parts': graph_of(12, both_ways([(i, i + 1, 1.0 + i / 7.0) for i in range(5)] +
                                               [(i, i + 1, 2.0 + i / 3.0) for i in range(6, 11)])),
         'h_order': graph_of(4, both_ways([(0, 1, 0.1), (1, 2, 0.2), (2, 3, 0.3)]))}
    for name, n in (('c_63', 63), ('d_64', 64), ('e_65', 65)):
        g[name] = graph_of(n, random_sparse(n, rng, n // 2))
    return g


def launch_distances(t, scans, max_nodes=None, tail=64):
    """sf_eval_distances over the CSR of `scans` of DistanceTable `t` into a fresh table with sentinels behind it."""
    from speaker_follower_amd import _lib
    arrays = t.in_edge_csr(scans)
    up = [torch.from_numpy(a).to(DEV) for a in arrays]
    table = torch.full((len(t.host) + tail,), SENTINEL, dtype=torch.float64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    g = _lib.EvalGraphs(len(scans), int(arrays[0][-1]), max_nodes or max(t.m[s] for s in scans), 0,
                        *[x.data_ptr() for x in up])
    status = _lib.lib.sf_eval_distances(C.byref(g), C.c_void_p(table.data_ptr()), C.c_void_p(err.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status, table.cpu().numpy(), int(err.item())


def test_distances_of_synthetic_graphs_in_one_launch_equal_dijkstra_bit_for_bit():
    from speaker_follower_amd import evaluation
    graphs = synthetic_graphs()
    t = evaluation.DistanceTable(graphs, device='cpu')             # (NavGraph.shortest: the host Dijkstra)
    assert t.dev is None and sorted(t.on_host) == sorted(graphs)
    status, got, err = launch_distances(t, t.scans)
    assert status == 0 and err == 0
    n = len(t.host)
    assert (got[n:] == SENTINEL).all()                             # nothing written behind the table
    for s in t.scans:
        m, o = t.m[s], t.off[s]
        assert (got[o:o + m * m] == t.host[o:o + m * m]).all(), s  # (==: to the last bit, inf == inf)
    assert np.isinf(t.host).any() and np.isinf(t.block('g_two_parts')).sum() == 72
    assert np.isinf(t.block('b_one_way')[1, 0]) and t.block('b_one_way')[0, 1] == 1.5
    D = t.block('h_order')                                          # symmetric weights, sums in the direction of travel
    assert D[0, 3] == (0.1 + 0.2) + 0.3 and D[3, 0] == (0.3 + 0.2) + 0.1 and D[0, 3] != D[3, 0]
    assert t.block('f_chain70')[0, 69] > 0 and np.isfinite(t.block('f_chain70')).all()


def test_distances_of_real_scans_equal_navgraph_shortest_bit_for_bit():
    from speaker_follower_amd import env, evaluation, nav_data
    geo = nav_data.load_geometry()
    largest = max(geo, key=lambda s: int(np.sum(geo[s]['included'])))
    assert int(np.sum(geo[largest]['included'])) == 348
    conn = nav_data.connectivity_dir(scans=[largest])
    graphs = {largest: env.NavGraph(os.path.join(conn, largest + '_connectivity.json'))}
    _, gold = r2r_world.load()
    for s in gold['config']['scans']:
        graphs['golden_' + s] = env.NavGraph(os.path.join(r2r_world.CONN, s + '_connectivity.json'))
    want = evaluation.DistanceTable(graphs, device='cpu')
    got = evaluation.DistanceTable(graphs, device=DEV)
    assert got.on_host == [] and got.dev is not None
    assert (got.host == want.host).all()
    assert (got.dev.cpu().numpy() == want.host).all()
    D = want.block(largest)
    assert D.shape == (348, 348) and (D != D.T).any()


# ------------------------------------------------------------------------------------------ the score kernel
BELOW_3 = math.nextafter(3.0, 0.0)


def score_world():
    """Two scans.  'A': goal v0; v1 at exactly 3.0 of it, v2 at the largest double below 3.0, v3 and v4 both at 2.5 (an
    oracle tie), v5 - v6 a component of their own (unreachable).  'B': a random graph."""
    rng = np.random.default_rng(9)
    A = graph_of(7, both_ways([(1, 0, 3.0), (2, 0, BELOW_3), (3, 0, 2.5), (4, 0, 2.5), (3, 4, 1.0), (1, 2, 10.0),
                               (1, 3, 7.0), (5, 6, 1.25)]))
    B = graph_of(9, random_sparse(9, rng, 5))
    return {'A': A, 'B': B}


def run_score_kernel(t, base, S, episodes, slots, n_slots):
    """episodes: per sample (scan, goal node, rows [S+1] local, actions [S]).  Returns the six arrays and err."""
    from speaker_follower_amd import _lib
    B = len(episodes)
    row = np.array([[base[sc] + r[k] for sc, _, r, _ in episodes] for k in range(S + 1)], np.int32)
    act = np.array([[a[k] for _, _, _, a in episodes] for k in range(S)], np.int64)
    per = dict(goal=np.array([base[sc] + g for sc, g, _, _ in episodes], np.int32),
               base=np.array([base[sc] for sc, _, _, _ in episodes], np.int32),
               m=np.array([t.m[sc] for sc, _, _, _ in episodes], np.int32),
               off=np.array([t.off[sc] for sc, _, _, _ in episodes], np.int64),
               slot=np.asarray(slots, np.int32))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                      # noqa: E731
    d = {k: up(v) for k, v in per.items()}
    row_d, act_d, table = up(row), up(act), up(t.host)
    f64 = torch.full((3, n_slots), SENTINEL, dtype=torch.float64, device=DEV)
    i32 = torch.full((3, n_slots), -9, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda x: x.data_ptr()                                                            # noqa: E731
    ep = _lib.EvalEpisodes(S, B, n_slots, 0, p(row_d), p(act_d), p(d['goal']), p(d['base']), p(d['m']), p(d['off']),
                           p(d['slot']), p(table), 3.0, p(f64[0]), p(f64[1]), p(f64[2]), p(i32[0]), p(i32[1]), p(i32[2]))
    _lib.call('sf_eval_score', C.byref(ep), C.c_void_p(err.data_ptr()),
              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return f64.cpu().numpy(), i32.cpu().numpy(), int(err.item())


def check_against_oracle(t, graphs, S, episodes, slots, n_slots):
    base = {'A': 100, 'B': 100 + t.m['A']}                     # (nav rows of a larger table: scan bases are not 0)
    f64, i32, err = run_score_kernel(t, base, S, episodes, slots, n_slots)
    assert err == 0
    gt, results = {}, {}
    for b, (sc, goal, rows, acts) in enumerate(episodes):
        stops = [k for k in range(S) if acts[k] == 0]
        n = stops[0] + 1 if stops else S
        gt[b] = dict(scan=sc, path=['v%d' % rows[0], 'v%d' % goal])
        results['%d_0' % b] = dict(trajectory=[('v%d' % r, 0.0, 0.0) for r in rows[:n + 1]])
    _, per_item = np_env.score_results(gt, graphs, results)
    used = set()
    for b, slot in enumerate(slots):
        if slot < 0:
            continue
        used.add(slot)
        w = per_item['%d_0' % b]
        assert (f64[0, slot], f64[1, slot], f64[2, slot]) == (w['nav_error'], w['oracle_error'], w['length']), b
        assert (i32[0, slot], bool(i32[1, slot]), bool(i32[2, slot])) == (w['steps'], w['success'], w['oracle_success']), b
    for slot in set(range(n_slots)) - used:                        # slot -1 rows and unused slots: sentinels intact
        assert (f64[:, slot] == SENTINEL).all() and (i32[:, slot] == -9).all()
    return per_item


def test_score_kernel_equals_the_oracle_bit_for_bit():
    from speaker_follower_amd import evaluation
    graphs = score_world()
    t = evaluation.DistanceTable(graphs, device='cpu')
    # S = 1, B = 1: a stop at step 0
    check_against_oracle(t, graphs, 1, [('A', 0, [3, 3], [0])], [0], 2)
    S = 6
    special = [
        ('A', 0, [3, 1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 0, 0]),       # ends at exactly 3.0: not a success (oracle: 2.5)
        ('A', 0, [1, 1, 1, 1, 1, 1, 1], [0, 2, 2, 2, 2, 2]),       # 3.0 throughout: neither flag
        ('A', 0, [1, 2, 2, 2, 2, 2, 2], [1, 0, 1, 1, 1, 1]),       # ends at the largest double below 3.0: a success
        ('A', 0, [1, 3, 4, 3, 1, 1, 1], [1, 1, 1, 1, 0, 1]),       # an oracle tie: v3 and v4 at 2.5
        ('A', 0, [5, 6, 5, 6, 5, 6, 5], [1, 1, 1, 1, 1, 1]),       # never stops (n = S); the goal is unreachable
        ('A', 5, [1, 2, 3, 4, 0, 1, 2], [3, 3, 3, 3, 3, 3]),       # unreachable the other way round
        ('A', 0, [4, 0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0]),       # reaches the goal: error 0.0
    ]
    rng = np.random.default_rng(3)
    episodes = list(special)
    while len(episodes) < 65:
        sc = 'AB'[int(rng.integers(2))]
        m = t.m[sc]
        rows = [int(x) for x in rng.integers(m, size=S + 1)]
        acts = [int(x) for x in rng.integers(0, 4, size=S)]
        episodes.append((sc, int(rng.integers(m)), rows, acts))
    slots = [int(x) for x in rng.permutation(70)[:65]]
    for b in (8, 20, 64):
        slots[b] = -1
    per_item = check_against_oracle(t, graphs, S, episodes, slots, 70)
    w = per_item
    assert w['0_0']['nav_error'] == 3.0 and not w['0_0']['success'] and w['0_0']['oracle_success']
    assert w['1_0']['oracle_error'] == 3.0 and not w['1_0']['oracle_success']
    assert w['2_0']['nav_error'] == BELOW_3 and w['2_0']['success']
    assert w['3_0']['oracle_error'] == 2.5
    assert math.isinf(w['4_0']['nav_error']) and not w['4_0']['success'] and not w['4_0']['oracle_success']
    assert w['4_0']['steps'] == S and math.isinf(w['5_0']['oracle_error'])
    # B = 1 at S = 6
    check_against_oracle(t, graphs, S, [special[3]], [1], 3)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_and_the_host_fill_above_the_lds_limit():
    from speaker_follower_amd import _lib, env, evaluation
    lib = _lib.lib
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sf_eval_distances(None, None, None, st) == _lib.SF_ERR_ARG
    assert lib.sf_eval_score(None, None, st) == _lib.SF_ERR_ARG
    assert lib.sf_eval_distances_bytes(None, 3) == 0
    assert lib.sf_eval_distances_bytes((C.c_int32 * 2)(3, -1), 2) == 0
    assert lib.sf_eval_distances_bytes((C.c_int32 * 2)(3, 348), -1) == 0
    assert lib.sf_eval_distances_bytes((C.c_int32 * 2)(3, 348), 2) == 8 * (9 + 348 * 348)
    one = torch.zeros(16, dtype=torch.float64, device=DEV)
    p = one.data_ptr()
    good = dict(n_scans=1, n_nodes=2, max_nodes=2, reserved=0, node_off=p, edge_off=p, edge_src=p, edge_w=p, dist_off=p)
    for bad in (dict(n_scans=-1), dict(n_nodes=-2), dict(max_nodes=-1), dict(max_nodes=3), dict(edge_w=None),
                dict(node_off=None)):
        g = _lib.EvalGraphs(**dict(good, **bad))
        assert lib.sf_eval_distances(C.byref(g), C.c_void_p(p), C.c_void_p(p), st) == _lib.SF_ERR_ARG, bad
    assert lib.sf_eval_distances(C.byref(_lib.EvalGraphs(**good)), None, C.c_void_p(p), st) == _lib.SF_ERR_ARG
    names = [f for f, _ in _lib.EvalEpisodes._fields_]
    ok = {f: (p if t is C.c_void_p else 1) for f, t in _lib.EvalEpisodes._fields_}
    ok['margin'] = 3.0
    for bad in [dict(S=-1), dict(B=-1), dict(n_slots=-1), dict(S=0)] + [{f: None} for f in names[4:12] + names[13:]]:
        e = _lib.EvalEpisodes(**dict(ok, **bad))
        assert lib.sf_eval_score(C.byref(e), C.c_void_p(p), st) == _lib.SF_ERR_ARG, bad
    assert lib.sf_eval_score(C.byref(_lib.EvalEpisodes(**ok)), None, st) == _lib.SF_ERR_ARG
    # a scan above the limit: SF_ERR_UNSUPPORTED, nothing launched; the Python side fills its block from the host
    assert lib.sf_eval_max_nodes() == 512
    _, gold = r2r_world.load()
    graphs = {s: env.NavGraph(os.path.join(r2r_world.CONN, s + '_connectivity.json')) for s in gold['config']['scans']}
    want = evaluation.DistanceTable(graphs, device='cpu')
    sizes = sorted(want.m.values())
    limit = sizes[len(sizes) // 2]                                  # (some scans above it, some not)
    assert sizes[0] <= limit < sizes[-1]
    lib.sf_debug_eval_max_nodes(limit)
    try:
        assert lib.sf_eval_max_nodes() == limit
        status, table, err = launch_distances(want, want.scans)
        assert status == _lib.SF_ERR_UNSUPPORTED and (table == SENTINEL).all()
        got = evaluation.DistanceTable(graphs, device=DEV)
    finally:
        lib.sf_debug_eval_max_nodes(0)
    assert lib.sf_eval_max_nodes() == 512
    assert sorted(got.on_host) == sorted(s for s in want.scans if want.m[s] > limit) and got.on_host
    assert (got.host == want.host).all() and (got.dev.cpu().numpy() == want.host).all()


# ------------------------------------------------------------------------------------------ score_agent
def make_agent(env, store, weights, episode_len, head=None):
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
    agent = agents.Seq2SeqAgent(env, '/tmp/sf_evaluation.json', enc, dec, episode_len=episode_len)
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
    weights = synth.follower_weights_peaky(cfg['weight_seed'])
    agent = make_agent(env, store, weights, cfg['episode_len'])
    agent.use_device_env(nav.NavTable(env, store))
    return dict(gold=gold, env=env, agent=agent, ev=evaluation.Evaluation(env=env), store=store, weights=weights,
                cfg=cfg)


@pytest.fixture(scope='module')
def val_seen_world():
    """The world of tests/test_gpu_r2r_val_seen.py: 782 instructions at batch 100, the g10b weights."""
    from speaker_follower_amd import evaluation, features, nav, synth
    items, _ = VS.load_items()
    gold = VS.load_sr_golden()
    cfg = gold['config']
    env, row_of, n = VS.build_env(items, batch_size=cfg['batch'], table_seed=cfg['table_seed'], scans=cfg['scans'])
    enc_w, dec_w = synth.follower_weights_peaky(cfg['weight_seed'])
    for k, v in gold['head'].items():
        dec_w[k] = np.asarray(v, np.float32).reshape(dec_w[k].shape)
    store = features.FeatureStore(env.host_table)
    agent = make_agent(env, store, (enc_w, dec_w), cfg['episode_len'])
    agent.use_device_env(nav.NavTable(env, store))
    return dict(gold=gold, env=env, agent=agent, ev=evaluation.Evaluation(env=env), store=store, cfg=cfg)


class Rewind:
    """The environment's item order and `random` as they were: two walks from the same state."""

    def __init__(self, env):
        self.env, self.data, self.state = env, list(env.data), random.getstate()

    def __call__(self):
        self.env.data[:] = self.data
        random.setstate(self.state)

    def after(self):
        return self.env.ix, [it['instr_id'] for it in self.env.data], random.random()


def by_test(w):
    """agent.test() + score_results(agent.results): (summary, scores, losses, results, where the walk ended)."""
    agent, ev = w['agent'], w['ev']
    results = agent.test(use_dropout=False, feedback='argmax')
    summary, scores = ev.score_results(results)
    return summary, {k: list(scores[k]) for k in LISTS}, list(agent.losses), results


def same_scores(got, want):
    for k in LISTS:
        assert list(got[k]) == list(want[k]), k                    # (== on floats: to the last bit, in the same order)


@pytest.mark.parametrize('name', ['g10_world', 'val_seen_world'])
def test_score_agent_equals_test_plus_score_results(name, request, monkeypatch):
    from speaker_follower_amd import nav
    w = request.getfixturevalue(name)
    agent, ev, env = w['agent'], w['ev'], w['env']
    rewind = Rewind(env)
    summary, scores, losses, results = by_test(w)
    end = rewind.after()
    made = []
    make = nav._Trajectory._make
    monkeypatch.setattr(nav._Trajectory, '_make', lambda self, key: made.append(key) or make(self, key))
    rewind()
    fallbacks, sweeps = ev.fallbacks, ev.sweeps
    got_summary, got_scores = ev.score_agent(agent)
    assert rewind.after() == end                                   # env.ix, the item order, the next random.random()
    assert ev.fallbacks == fallbacks and ev.sweeps == sweeps + 1
    assert ev.last_host_syncs == 1
    assert made == [] and agent.results == {}
    same_scores(got_scores, scores)
    assert got_summary == summary and set(got_summary) == set(SUMMARY) | {'model_score'}
    assert agent.losses == losses
    print('%s: %d instructions in %d minibatches, success_rate %.4f, one host sync'
          % (name, len(got_scores['nav_errors']), len(losses), got_summary['success_rate']))
    # keep_results: the lazy result objects of test(), in its order
    rewind()
    kept_summary, kept_scores = ev.score_agent(agent, keep_results=True)
    assert ev.last_host_syncs == 1 and made == []
    assert kept_summary == summary
    same_scores(kept_scores, scores)
    assert list(agent.results) == list(results)
    for k, r in results.items():
        assert agent.results[k] == r, k
    rewind()


def test_success_rate_parity_with_the_reference_stack_through_score_agent(val_seen_world):
    w = val_seen_world
    agent, ev, gold = w['agent'], w['ev'], w['gold']
    rewind = Rewind(w['env'])
    summary, scores = ev.score_agent(agent, keep_results=True)
    rewind()
    order = [k for k in agent.results if k in ev.instr_ids]
    assert len(order) == 780 == len(scores['nav_errors'])
    differ = []
    for i, k in enumerate(order):
        want = gold['items'][k]
        if [p[0] for p in agent.results[k]['trajectory']] != want['viewpoints']:
            differ.append(k)
            continue
        got = [scores[name][i] for name in LISTS]
        np.testing.assert_allclose([got[0], got[1], got[3]], [want['nav_error'], want['oracle_error'], want['length']],
                                   rtol=1e-9)
        assert (got[2], got[4], got[5]) == (want['steps'], want['success'], want['oracle_success']), k
    print('trajectories that differ from the reference: %d; success_rate %.6f (reference %.6f)'
          % (len(differ), summary['success_rate'], gold['summary']['success_rate']))
    assert all(gold['items'][k]['min_margin'] < 1e-3 for k in differ), differ
    if not differ:
        for k in SUMMARY:
            np.testing.assert_allclose(summary[k], gold['summary'][k], rtol=1e-9)
        assert summary['success_rate'] == 65 / 780


@pytest.mark.parametrize('case', ['test_graph_off', 'sample'])
def test_score_agent_falls_back_where_the_graph_rollout_does_not_apply(g10_world, case):
    w = g10_world
    agent, ev = w['agent'], w['ev']
    rewind = Rewind(w['env'])
    summary, scores, losses, _ = by_test(w)
    rewind()
    before = ev.fallbacks
    try:
        if case == 'test_graph_off':
            agent.test_graph = False
            got_summary, got_scores = ev.score_agent(agent)
        else:
            got_summary, got_scores = ev.score_agent(agent, feedback='sample')
    finally:
        agent.__dict__.pop('test_graph', None)
    assert ev.fallbacks == before + 1
    again, again_scores = ev.score_results(agent.results)          # what the fall-back scored is what test() left
    assert got_summary == again
    same_scores(got_scores, again_scores)
    if case == 'test_graph_off':                                   # (the eager rollout pads instructions to the minibatch's
        for k in ('trajectory_steps', 'success', 'oracle_success', 'nav_errors'):   # longest: the same walk on this world)
            assert list(got_scores[k]) == list(scores[k]), k
    rewind()


def test_score_agent_never_scores_a_faulting_sweep(g10_world):
    """Every persistent launch of a fresh agent's captured rollout gives up its first wait (sf_debug_persist_timeout(0)
    at capture time: the bound is a kernel argument): the sweep reads the raised fault word at its one sync, scores
    nothing and runs agent.test(), whose rollouts are repaired on the per-step kernels."""
    from speaker_follower_amd import _lib, runtime
    w = g10_world
    ev = w['ev']
    rewind = Rewind(w['env'])
    summary, scores, losses, _ = by_test(w)
    end = rewind.after()
    rewind()
    agent = make_agent(w['env'], w['store'], w['weights'], w['cfg']['episode_len'])
    agent.use_device_env(w['agent'].nav_table)
    before = ev.fallbacks
    runtime.take_fault(DEV)
    _lib.lib.sf_debug_persist_timeout(0)
    try:
        got_summary, got_scores = ev.score_agent(agent)
    finally:
        _lib.lib.sf_debug_persist_timeout(-1)
        torch.cuda.synchronize()
        runtime.take_fault(DEV)
        agent.__dict__.pop('_test_graphs', None)
    assert ev.fallbacks == before + 1 and agent._engine.fallbacks >= 1
    assert rewind.after() == end                                   # (the faulting sweep's walk was undone: ONE walk)
    same_scores(got_scores, scores)                                # the same walk, scored once, from healthy rollouts
    for k in SUMMARY:
        assert got_summary[k] == summary[k]
    rewind()
