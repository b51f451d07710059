"""Shared by tests/test_path_metrics_host.py and tests/test_gpu_path_metrics.py (no tests of its own): the published
definitions of SPL, nDTW and SDTW restated in plain Python over a distance block and LOCAL node lists, small synthetic
graphs, and the case list both files score.

    P = p_0 .. p_n the visited nodes, R = r_0 .. r_{g-1} the gold path, D[src][dst] the scan's distances, margin 3.0
    shortest = D[p_0][r_{g-1}]
    dtw      = C[n+1][g], C[0][0] = 0, C[a][0] = C[0][b] = inf, C[a][b] = D[p_{a-1}][r_{b-1}] + min(up, left, diagonal)
    spl      = 0 unless success, else 1 if max(length, shortest) == 0, else shortest / max(length, shortest)
    ndtw     = exp(-dtw / (g * margin)) with math.exp, sdtw = ndtw if success else 0

The recurrence is run ROW BY ROW here.  Every cell is one rounded add of one table element to an exact minimum, so any
other schedule (the kernel's anti-diagonals) must give the same bits: the tests compare with ==."""
import math

import numpy as np

MARGIN = 3.0
FIELDS = ('nav_error', 'oracle_error', 'trajectory_steps', 'trajectory_length', 'success', 'oracle_success',
          'shortest_length', 'dtw', 'spl', 'ndtw', 'sdtw')
PATH_LISTS = ('shortest_lengths', 'dtw', 'spl', 'ndtw', 'sdtw')


def dtw_of(D, P, R, transposed=False):
    inf = math.inf
    n1, g = len(P), len(R)
    Ct = [[inf] * (g + 1) for _ in range(n1 + 1)]
    Ct[0][0] = 0.0
    for a in range(1, n1 + 1):
        for b in range(1, g + 1):
            cost = float(D[R[b - 1]][P[a - 1]]) if transposed else float(D[P[a - 1]][R[b - 1]])
            Ct[a][b] = cost + min(Ct[a - 1][b], Ct[a][b - 1], Ct[a - 1][b - 1])
    return Ct[n1][g]


def restate(D, P, R, margin=MARGIN):
    """The eleven values of one result, in FIELDS order."""
    goal = R[-1]
    to_goal = [float(D[p][goal]) for p in P]
    nav_error, oracle_error = to_goal[-1], to_goal[0]
    for d in to_goal:
        if d < oracle_error:
            oracle_error = d
    length = 0.0
    for u, v in zip(P[:-1], P[1:]):
        length += float(D[u][v])
    success = nav_error < margin
    shortest = float(D[P[0]][goal])
    dtw = dtw_of(D, P, R)
    if not success:
        spl = 0.0
    elif max(length, shortest) == 0:
        spl = 1.0
    else:
        spl = shortest / max(length, shortest)
    ndtw = math.exp(-dtw / (len(R) * margin))
    return (nav_error, oracle_error, len(P) - 1, length, success, oracle_error < margin, shortest, dtw, spl, ndtw,
            ndtw if success else 0.0)


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
    edges = [(i, int(rng.integers(i)), float(rng.uniform(0.3, 4.0))) for i in range(1, n)]
    for _ in range(extra):
        u, v = (int(x) for x in rng.integers(n, size=2))
        if u != v:
            edges.append((u, v, float(rng.uniform(0.3, 4.0))))
    return both_ways(edges)


def graphs():
    rng = np.random.default_rng(17)
    return {'a_single': graph_of(1, []),
            'b_line6': graph_of(6, both_ways([(i, i + 1, 1.0) for i in range(5)])),                 # unit weights: ties
            'c_order': graph_of(4, both_ways([(0, 1, 0.1), (1, 2, 0.2), (2, 3, 0.3)])),             # h_order's weights
            'd_two_parts': graph_of(12, both_ways([(i, i + 1, 1.0 + i / 7.0) for i in range(5)] +
                                                  [(i, i + 1, 2.0 + i / 3.0) for i in range(6, 11)])),
            'e_rand70': graph_of(70, random_sparse(70, rng, 35)),
            'f_grid9': graph_of(9, both_ways([(r * 3 + c, r * 3 + c + 1, 1.0) for r in range(3) for c in range(2)] +
                                             [(r * 3 + c, r * 3 + c + 3, 1.0) for r in range(2) for c in range(3)]))}


# the issue's known answers on the unit line graph: (R, P, dtw, ndtw, success, spl, sdtw) -- None: not stated
KNOWN = [([0, 1, 2, 3], [0, 1, 2, 3], 0.0, 1.0, True, 1.0, None),
         ([0, 1, 2, 3], [0], 6.0, math.exp(-0.5), False, 0.0, 0.0),
         ([0, 1, 2, 3], [0, 1, 2, 3, 4, 5], 3.0, math.exp(-0.25), True, 3.0 / 5.0, None),
         ([0], [0, 1, 2, 3], 6.0, math.exp(-2.0), None, None, None)]

N_CASES = 257


def cases():
    """[(scan, P, R)] with P[0] == R[0], local node indices: the known answers, the edges the issue lists (gold paths
    of 1, 2, 63 and 64 nodes, routes of 1, 2, 64, 65 and 130 poses, a scan of one node, inf distances, ties among all
    three predecessors), then random routes up to N_CASES."""
    rng = np.random.default_rng(23)
    walk = lambda m, k, start: [start] + [int(x) for x in rng.integers(m, size=k - 1)]    # noqa: E731
    out = [('b_line6', P, R) for R, P, _, _, _, _, _ in KNOWN]
    out += [('a_single', [0], [0]),                                   # start == goal, an immediate stop: spl 1.0
            ('a_single', [0, 0, 0], [0]),
            ('c_order', [0], [0, 3]),                                 # sums that depend on the direction of travel:
            ('c_order', [0, 1, 0], [0, 3]),                           # D[0][3] = (.1 + .2) + .3 != D[3][0] = (.3 + .2) + .1
            ('c_order', [0, 3, 2, 1], [0, 1, 2, 3]),
            ('c_order', [3, 0], [3, 2, 1, 0]),
            ('d_two_parts', [0, 1, 2], [0, 7, 8]),                    # gold nodes in the other component: dtw inf
            ('d_two_parts', [0, 7, 1], [0, 1, 2]),                    # a pose there: an inf cost on the way, length inf
            ('d_two_parts', [0, 1], [0, 1, 9]),                       # the goal unreachable: shortest inf, never a success
            ('f_grid9', [0, 1, 4, 5, 8], [0, 3, 4, 7, 8]),            # unit grid: ties among up, left and diagonal
            ('f_grid9', [0, 3, 6, 7, 8, 5, 2, 1, 0], [0, 4, 8])]
    for g in (1, 2, 63, 64):
        for k in (1, 2, 64, 65, 130):
            R = walk(70, g, int(rng.integers(70)))
            out.append(('e_rand70', walk(70, k, R[0]), R))
    sizes = {'b_line6': 6, 'c_order': 4, 'd_two_parts': 12, 'e_rand70': 70, 'f_grid9': 9}
    names = sorted(sizes)
    while len(out) < N_CASES:
        s = names[int(rng.integers(len(names)))]
        R = walk(sizes[s], int(rng.integers(1, 9)), int(rng.integers(sizes[s])))
        P = walk(sizes[s], int(rng.integers(1, 12)), R[0])
        if s == 'd_two_parts':                   # a route cannot leave its start's component (nodes 0-5 / 6-11): a goal
            P = [p % 6 + 6 * (R[0] // 6) for p in P]                 # in the other one is then never a success
        out.append((s, P, R))
    return out


def evaluation_of(the_cases, the_graphs, **kw):
    """An Evaluation whose ground truth is the cases' gold paths (path_id = case index), and their results."""
    from speaker_follower_amd import evaluation
    items = [dict(path_id=i, scan=s, path=['v%d' % r for r in R]) for i, (s, _, R) in enumerate(the_cases)]
    ev = evaluation.Evaluation(items=items, graphs=the_graphs, **kw)
    ev.instr_ids = {'%d_0' % i for i in range(len(items))}           # one result per case
    results = {'%d_0' % i: dict(instr_id='%d_0' % i, trajectory=[('v%d' % p, 0.0, 0.0) for p in P])
               for i, (_, P, _) in enumerate(the_cases)}
    return ev, results
