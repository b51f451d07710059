"""Scoring of navigation results (tasks/R2R/eval.py:23-139): navigation error = shortest-path distance from the LAST
viewpoint of a trajectory to the goal, oracle error = from the closest viewpoint on it, success = error < 3 m, the
summary averages over the instructions '<path_id>_0' .. '_2' of the split.

  * `DistanceTable`   the all-pairs distances of a set of scans as ONE float64 table, scan blocks back to back,
                      D[src][dst] over the INCLUDED viewpoints in connectivity-file order (the local order of
                      nav.NavTable's rows).  Built once: by sf_eval_distances (csrc/sf_eval.hip) when a GPU is
                      present, else from env.NavGraph.shortest -- the same numbers to the last bit,
                      source-major: D[a][b] and D[b][a] differ in their last bits for half of all pairs.
  * `Evaluation`      eval.py's class: `_score_item`, `score_results`, `score_file` with the reference's contract, and
                      `score_agent`: agent.test() + score_results as one device sweep with one host sync.
                      `path_metrics=True` adds SPL, nDTW and SDTW (no reference counterpart: their published
                      definitions) through sf_eval_score_routes (csrc/sf_eval_routes.hip);
                      `score_routes` scores a batch of routes in one launch.
                      `coverage_metrics=True` adds CLS (coverage weighted by length score) on top of those: the
                      per-gold-node minimum distance comes out of the same launch (sf_eval_score_routes_coverage).
                      For a baseline agent (agents.StopAgent / ShortestAgent / RandomAgent) `score_agent` is one
                      sf_nav_walk launch over the split and one route-scoring launch behind it.
  * `evaluate_simple_agents`, `eval_simple_agents`   eval.py:148-163, the Stop / Shortest / Random table.

The reference takes its table from networkx (all_pairs_dijkstra_path_length); nothing here imports it.
"""
import ctypes as C
import json
import math
import os
import random
from collections import defaultdict, namedtuple

import numpy as np

EvalResult = namedtuple('EvalResult', 'nav_error, oracle_error, trajectory_steps, trajectory_length, success, '
                                      'oracle_success')                                          # eval.py:18-20

PathEvalResult = namedtuple('PathEvalResult', EvalResult._fields + ('shortest_length', 'dtw', 'spl', 'ndtw', 'sdtw'))

CoverageEvalResult = namedtuple('CoverageEvalResult', PathEvalResult._fields + ('gold_length', 'coverage', 'length_score',
                                                                               'cls'))

DATA_JSON = 'tasks/R2R/data/R2R_%s.json'                                 # utils.py:54-59
CONNECTIVITY = 'connectivity'

_LISTS = ('nav_errors', 'oracle_errors', 'trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success')
_PATH_LISTS = ('shortest_lengths', 'dtw', 'spl', 'ndtw', 'sdtw')
_COVERAGE_LISTS = ('gold_lengths', 'coverage', 'length_score', 'cls')


def path_metrics_of(r, shortest, dtw, gold_nodes, margin):
    """EvalResult `r` + the two device quantities -> PathEvalResult.  THE place where spl, ndtw
    and sdtw are formed, for the host and the device path alike, per item and with math.exp (np.exp may differ in the
    last bit).  An unreachable goal has shortest = inf and is never a success: no inf / inf is formed."""
    if not r.success:
        spl = 0.0
    else:
        longest = max(r.trajectory_length, shortest)
        spl = 1.0 if longest == 0 else shortest / longest
    ndtw = math.exp(-dtw / (gold_nodes * margin))
    return PathEvalResult(*r, shortest_length=shortest, dtw=dtw, spl=spl, ndtw=ndtw, sdtw=ndtw if r.success else 0.0)


def coverage_metrics_of(r, near, gold_length, margin):
    """PathEvalResult `r` + near[b] = min over the poses of D[pose][gold node b] + the gold path's length ->
    CoverageEvalResult.  THE place where coverage, length_score and cls are formed, for the host
    and the device path alike: the sum runs left to right in gold order with math.exp on Python floats.  A gold node no
    pose reaches (near = inf) contributes 0.0; a gold path nobody can walk scores 0.0: no inf / inf is formed."""
    total = 0.0
    for d in near:
        total = total + (0.0 if d == math.inf else math.exp(-d / margin))
    coverage = total / len(near)
    expected = coverage * gold_length
    if gold_length == math.inf:
        length_score = 0.0
    else:
        spread = expected + abs(expected - r.trajectory_length)
        length_score = 1.0 if spread == 0 else expected / spread
    return CoverageEvalResult(*r, gold_length=gold_length, coverage=coverage, length_score=length_score,
                              cls=coverage * length_score)


def dtw_rows(cost):
    """C[n+1][g] of the warping recurrence over cost[a][b] = D[p_a][r_b] (lists of float), row by row: every cell is
    one rounded add of one table element to an exact three-way minimum (sf_eval_score_routes runs the anti-diagonals:
    the same bits)."""
    inf = math.inf
    prev = [0.0] + [inf] * len(cost[0])
    for row in cost:
        cur = [inf]
        for b, c in enumerate(row):
            cur.append(c + min(prev[b + 1], cur[b], prev[b]))
        prev = cur
    return prev[-1]


class DistanceTable:
    """scan -> m x m float64 block D[src][dst] of one flat table (`host`; `dev` when it was built on the device)."""

    def __init__(self, graphs, device=None):
        """graphs: scan -> env.NavGraph.  device: where to build the table and keep it (None: the current GPU when there
        is one, else 'cpu': NavGraph.shortest, host copy only)."""
        self.scans = sorted(graphs)
        self.graphs = graphs
        self.nodes, self.index, self.m, self.off = {}, {}, {}, {}
        total = 0
        for s in self.scans:
            g = graphs[s]
            nodes = [v for v, inc in zip(g.ids, g.included) if inc]
            self.nodes[s], self.index[s] = nodes, {v: i for i, v in enumerate(nodes)}
            self.m[s], self.off[s] = len(nodes), total
            total += len(nodes) ** 2
        self.host = np.full(total, np.inf, np.float64)
        self.dev = None
        self.on_host = []                                    # scans whose block came from NavGraph.shortest
        import torch
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else 'cpu'
        device = torch.device(device)
        if device.type == 'cuda' and total:
            self._build_on_device(device)
        else:
            for s in self.scans:
                self._fill_from_host(s)

    def block(self, scan):
        m = self.m[scan]
        return self.host[self.off[scan]:self.off[scan] + m * m].reshape(m, m)

    def _fill_from_host(self, scan):
        """The scan's block from NavGraph.shortest(src): Dijkstra accumulating d + w outward from the source."""
        g, ix, D = self.graphs[scan], self.index[scan], self.block(scan)
        for i, v in enumerate(self.nodes[scan]):
            for u, d in g.shortest(v)[0].items():
                D[i, ix[u]] = d
        self.on_host.append(scan)

    def in_edge_csr(self, scans):
        """The in-edge CSR sf_eval_distances reads (include/sf_hip.h: sf_eval_graphs) of `scans`, as host arrays."""
        node_off, edge_off, src, w, dist_off = [0], [0], [], [], []
        for s in scans:
            ix, into = self.index[s], {v: [] for v in self.nodes[s]}
            for u, nb in self.graphs[s].adj.items():
                for v, wt in nb.items():
                    into[v].append((ix[u], wt))
            for v in self.nodes[s]:
                src += [u for u, _ in into[v]]
                w += [wt for _, wt in into[v]]
                edge_off.append(len(src))
            node_off.append(node_off[-1] + self.m[s])
            dist_off.append(self.off[s])
        return (np.asarray(node_off, np.int32), np.asarray(edge_off, np.int32), np.asarray(src, np.int32),
                np.asarray(w, np.float64), np.asarray(dist_off, np.int64))

    def _build_on_device(self, device):
        import torch
        from . import _lib
        from .runtime import stream
        limit = _lib.lib.sf_eval_max_nodes()
        small = [s for s in self.scans if 0 < self.m[s] <= limit]
        with torch.cuda.device(device):
            self.dev = torch.full((len(self.host),), float('inf'), dtype=torch.float64, device=device)
            if small:
                arrays = self.in_edge_csr(small)
                up = [torch.from_numpy(a).to(device) for a in arrays]
                err = torch.zeros(1, dtype=torch.int32, device=device)
                g = _lib.EvalGraphs(len(small), int(arrays[0][-1]), max(self.m[s] for s in small), 0,
                                    *[t.data_ptr() for t in up])
                _lib.call('sf_eval_distances', C.byref(g), C.c_void_p(self.dev.data_ptr()),
                          C.c_void_p(err.data_ptr()), stream())
                self.host[:] = self.dev.cpu().numpy()
                if int(err.item()):
                    raise RuntimeError('sf_eval_distances: a graph did not settle in as many rounds as it has nodes '
                                       '(an edge weight that is not positive?)')
            big = [s for s in self.scans if self.m[s] > limit]
            for s in big:                                    # above the kernel's LDS budget: this block from the host
                self._fill_from_host(s)
            if big:
                self.dev.copy_(torch.from_numpy(self.host))


def _load_graphs(scans, nav_graph_path=CONNECTIVITY):
    from .env import NavGraph
    return {s: NavGraph(os.path.join(nav_graph_path, s + '_connectivity.json')) for s in sorted(scans)}


class Evaluation(object):
    """eval.py:23-139.  Results: {instr_id: {'instr_id', 'trajectory': [(viewpoint_id, heading, elevation), ...]}}.

    Evaluation(splits)                 reads tasks/R2R/data/R2R_<split>.json and connectivity/ relative to the working
                                       directory, as compat/env.py does (the reference's form)
    Evaluation(env=env)                the items and graphs of an env.R2RIndexEnv / compat R2RBatch
    Evaluation(items=..., graphs=...)  items with 'path_id', 'scan', 'path'; graphs: scan -> env.NavGraph

    path_metrics=True adds the path-fidelity measures (no reference counterpart): `_score_item` and
    `score_routes` return PathEvalResult (EvalResult's fields, then shortest_length, dtw, spl, ndtw, sdtw), `scores`
    gains the lists 'shortest_lengths', 'dtw', 'spl', 'ndtw', 'sdtw' and the summary 'spl', 'ndtw', 'sdtw'.  With the
    distance table on the device every batch of results is ONE sf_eval_score_routes launch (csrc/sf_eval_routes.hip)
    and one host sync, else the host loop: the same values to the last bit.

    coverage_metrics=True turns path_metrics on and adds CLS (Jain et al. 2019): the results are
    CoverageEvalResult (PathEvalResult's fields, then gold_length, coverage, length_score, cls), `scores` gains the
    lists 'gold_lengths', 'coverage', 'length_score', 'cls' and the summary 'cls'.  The launch is then
    sf_eval_score_routes_coverage: the same one, which also leaves the least distance to every gold node."""

    def __init__(self, splits=None, env=None, items=None, graphs=None, nav_graph_path=CONNECTIVITY, device=None,
                 path_metrics=False, coverage_metrics=False):
        self.error_margin = 3.0
        self.coverage_metrics = bool(coverage_metrics)
        self.path_metrics = bool(path_metrics) or self.coverage_metrics
        self._gold = self._gold_len = None
        if env is not None:
            items = list(env.data) if items is None else items
            graphs = env.graphs if graphs is None else graphs
            splits = list(getattr(env, 'splits', [])) if splits is None else splits
        elif items is None:
            items = []
            for split in splits:
                with open(DATA_JSON % split) as f:
                    items += json.load(f)
        self.splits = list(splits) if splits is not None else []
        self.gt, self.instr_ids, self.scans = {}, [], []
        for item in items:
            if item['path_id'] in self.gt:                   # (an env holds one item per instruction)
                continue
            self.gt[item['path_id']] = item
            self.scans.append(item['scan'])
            self.instr_ids += ['%d_%d' % (item['path_id'], i) for i in range(3)]                  # eval.py:36-38
        self.scans = set(self.scans)
        self.instr_ids = set(self.instr_ids)
        self._graphs_given, self._nav_graph_path, self._device = graphs, nav_graph_path, device
        self._table = None
        self._checked_navs = {}
        self.fallbacks = 0
        self.host_syncs = self.last_host_syncs = self.sweeps = 0
        self._sweep_buffers = {}

    # ---- distances: built once, on first use
    @property
    def graphs(self):
        if self._graphs_given is None:
            self._graphs_given = _load_graphs(self.scans, self._nav_graph_path)
        return self._graphs_given

    @property
    def table(self):
        if self._table is None:
            graphs = self.graphs
            self._table = DistanceTable({s: graphs[s] for s in self.scans}, device=self._device)
        return self._table

    def distance(self, scan, a, b):
        """eval.py's distances[scan][a][b]: FROM a TO b."""
        t = self.table
        return float(t.block(scan)[t.index[scan][a], t.index[scan][b]])

    # ---- eval.py:46-84
    def _score_rows(self, scan, rows, goal, gold=None, gold_length=None):
        """One path as LOCAL node indices of its scan (`gold`: the gold path likewise, with path_metrics; `gold_length`:
        its length, with coverage_metrics)."""
        r = self._score_six(scan, rows, goal)
        if not self.path_metrics:
            return r
        D = self.table.block(scan)
        if not self.coverage_metrics:
            return path_metrics_of(r, float(D[rows[0], goal]), dtw_rows(D[np.ix_(rows, gold)].tolist()), len(gold),
                                   self.error_margin)
        cost = D[np.ix_(rows, gold)].tolist()
        r = path_metrics_of(r, float(D[rows[0], goal]), dtw_rows(cost), len(gold), self.error_margin)
        return coverage_metrics_of(r, [min(col) for col in zip(*cost)], gold_length, self.error_margin)

    def _score_six(self, scan, rows, goal):
        D = self.table.block(scan)
        to_goal = D[rows, goal].tolist()
        nav_error, oracle_error = to_goal[-1], to_goal[0]
        for d in to_goal:                                    # the first minimum (eval.py:46-54)
            if d < oracle_error:
                oracle_error = d
        length = 0
        for d in D[rows[:-1], rows[1:]].tolist():            # in path order (eval.py:69-73)
            length += d
        return EvalResult(nav_error=nav_error, oracle_error=oracle_error, trajectory_steps=len(rows) - 1,
                          trajectory_length=length, success=nav_error < self.error_margin,
                          oracle_success=oracle_error < self.error_margin)

    def _score_item(self, instr_id, path):
        gt = self.gt[int(instr_id.split('_')[0])]
        assert gt['path'][0] == path[0][0], 'Result trajectories should include the start position'
        ix = self.table.index[gt['scan']]
        return self._score_rows(gt['scan'], np.fromiter((ix[p[0]] for p in path), np.int64, len(path)),
                                ix[gt['path'][-1]], [ix[v] for v in gt['path']] if self.path_metrics else None,
                                self._gold_lengths()[gt['path_id']] if self.coverage_metrics else None)

    def _local_rows(self, nav, scan):
        """First nav row of `scan` in `nav`, after checking ONCE that the table's rows of that scan are this table's
        nodes in this table's order."""
        key = (id(nav), scan)
        if key not in self._checked_navs:
            t, b = self.table, nav.base[scan]
            if [v for _, v in nav.vp_of[b:b + nav.scan_rows[scan]]] != t.nodes[scan]:
                raise ValueError('the navigation table orders the viewpoints of scan %s differently' % scan)
            self._checked_navs[key] = (nav, b)               # (nav kept alive: the key holds its id)
        return self._checked_navs[key][1]

    def _score_device_results(self, found):
        """[(instr_id, result of a device rollout)] -> EvalResults, from the integer nav rows the results hold:
        vectorised look-ups into the host table, no 'trajectory' built."""
        t = self.table
        N = len(found)
        paths = [res.nav_rows() for _, res in found]
        n = np.array([len(r) - 1 for _, r in paths], np.int64)
        L = int(n.max()) + 1
        local = np.zeros((N, L), np.int64)                   # local node index of every pose, the last one repeated
        goal, m, off = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
        for i, ((instr_id, _), (nav, rows)) in enumerate(zip(found, paths)):
            gt = self.gt[int(instr_id.split('_')[0])]
            scan = gt['scan']
            assert nav.row_of[(scan, gt['path'][0])] == rows[0], 'Result trajectories should include the start position'
            local[i, :len(rows)] = np.asarray(rows, np.int64) - self._local_rows(nav, scan)
            local[i, len(rows):] = local[i, len(rows) - 1]
            m[i], off[i], goal[i] = t.m[scan], t.off[scan], t.index[scan][gt['path'][-1]]
        if (local < 0).any() or (local >= m[:, None]).any():
            raise ValueError('a result holds a nav row outside its scan')
        every = np.arange(N)
        row_at = off[:, None] + local * m[:, None]                                 # element of D[pose][0]
        to_goal = t.host[row_at + goal[:, None]]                                   # [N, L]
        nav_error = to_goal[every, n]
        on_path = np.arange(L)[None, :] <= n[:, None]
        oracle_error = np.where(on_path, to_goal, np.inf).min(1)                   # (the value of the first minimum)
        length = np.zeros(N, np.float64)
        for s in range(L - 1):                                                     # in path order (eval.py:69-73)
            length = length + np.where(s < n, t.host[row_at[:, s] + local[:, s + 1]], 0.0)
        margin = self.error_margin
        return [EvalResult(a, b, c, d, a < margin, b < margin)
                for a, b, c, d in zip(nav_error.tolist(), oracle_error.tolist(), n.tolist(), length.tolist())]

    # ---- batches of routes: one sf_eval_score_routes launch (csrc/sf_eval_routes.hip), or the host loop
    def _gold_table(self):
        """The gold paths as the ragged table of LOCAL node indices sf_eval_score_routes reads: path_id -> its index,
        offsets, nodes, the longest path; uploaded once per Evaluation when the distances are on the device."""
        if self._gold is None:
            t = self.table
            ids, off, node = {}, [0], []
            for pid, gt in self.gt.items():
                ids[pid] = len(ids)
                node += [t.index[gt['scan']][v] for v in gt['path']]
                off.append(len(node))
            gold = dict(ids=ids, off=np.asarray(off, np.int32), node=np.asarray(node, np.int32),
                        longest=int(np.diff(off).max()) if ids else 0, dev=None)
            if t.dev is not None and node:
                import torch
                gold['dev'] = tuple(torch.from_numpy(gold[k]).to(t.dev.device) for k in ('off', 'node'))
            self._gold = gold
        return self._gold

    def _gold_lengths(self):
        """path_id -> the length of its gold path: the edges D[r_k][r_k+1] of the HOST table added left to right in path
        order (0.0 for a path of one node).  Static per gold path: formed once per Evaluation."""
        if self._gold_len is None:
            t, out = self.table, {}
            for pid, gt in self.gt.items():
                D, ix = t.block(gt['scan']), t.index[gt['scan']]
                nodes = [ix[v] for v in gt['path']]
                length = 0.0
                for d in D[nodes[:-1], nodes[1:]].tolist():
                    length = length + d
                out[pid] = length
            self._gold_len = out
        return self._gold_len

    def _route_of(self, instr_id, result):
        """(ground truth, the poses as LOCAL node indices) of a trajectory [(viewpoint, heading, elevation), ...] or of
        a result of a device rollout, with the reference's assertion on the start."""
        gt = self.gt[int(instr_id.split('_')[0])]
        scan = gt['scan']
        if hasattr(result, 'nav_rows'):
            nav, rows = result.nav_rows()
            assert nav.row_of[(scan, gt['path'][0])] == rows[0], 'Result trajectories should include the start position'
            local = np.asarray(rows, np.int64) - self._local_rows(nav, scan)
            if (local < 0).any() or (local >= self.table.m[scan]).any():
                raise ValueError('a result holds a nav row outside its scan')
            return gt, local
        assert gt['path'][0] == result[0][0], 'Result trajectories should include the start position'
        ix = self.table.index[scan]
        return gt, np.fromiter((ix[p[0]] for p in result), np.int64, len(result))

    def _score_routes(self, routes):
        """[(ground truth, local poses)] -> results of this evaluator's type: ONE ragged launch and one host sync when
        the distances are on the device, else -- and where the kernel refuses (`fallbacks`) -- the host loop."""
        out = self._score_routes_on_device(routes) if routes and self.table.dev is not None else None
        if out is None:
            t = self.table
            out = []
            for gt, rows in routes:
                ix = t.index[gt['scan']]
                out.append(self._score_rows(gt['scan'], rows, ix[gt['path'][-1]],
                                            [ix[v] for v in gt['path']] if self.path_metrics else None,
                                            self._gold_lengths()[gt['path_id']] if self.coverage_metrics else None))
        return out

    def _score_routes_on_device(self, routes):
        import torch
        from . import _lib
        from .runtime import stream
        t, gold = self.table, self._gold_table()
        if gold['dev'] is None:
            return None
        dev = t.dev.device
        N = len(routes)
        n = np.array([len(rows) - 1 for _, rows in routes], np.int64)
        i32 = np.zeros((5, N), np.int32)                     # n_steps, gold_id, m, slot, scan_base (0: poses are local)
        i64 = np.zeros((2, N), np.int64)                     # row_first, dist_off
        i32[0], i32[3] = n, np.arange(N)
        i64[0, 1:] = np.cumsum(n[:-1] + 1)
        for i, (gt, _) in enumerate(routes):
            i32[1, i], i32[2, i], i64[1, i] = gold['ids'][gt['path_id']], t.m[gt['scan']], t.off[gt['scan']]
        poses = np.concatenate([rows for _, rows in routes]).astype(np.int32)
        ptr_of = lambda x: x.data_ptr()                       # noqa: E731
        with torch.cuda.device(dev):
            d32, d64, rows_d = (torch.from_numpy(a).to(dev) for a in (i32, i64, poses))
            o64 = torch.empty(5, N, dtype=torch.float64, device=dev)
            o32 = torch.zeros(3 * N + 1, dtype=torch.int32, device=dev)                   # (the last word: err)
            e = _lib.EvalRoutes(0, N, N, 1, len(gold['ids']), len(gold['node']), gold['longest'], 0, len(poses),
                                ptr_of(rows_d), ptr_of(d64[0]), ptr_of(d32[0]), None, ptr_of(gold['dev'][0]),
                                ptr_of(gold['dev'][1]), ptr_of(d32[1]), ptr_of(d32[4]), ptr_of(d32[2]), ptr_of(d64[1]),
                                ptr_of(d32[3]), ptr_of(t.dev), self.error_margin, *[ptr_of(o64[k]) for k in range(5)],
                                *[ptr_of(o32[k * N:]) for k in range(3)])
            if self.coverage_metrics:                         # the same launch, + near [N, longest]
                entry, ld = 'sf_eval_score_routes_coverage', gold['longest']
                near = torch.empty(N, ld, dtype=torch.float64, device=dev)
                status = _lib.lib.sf_eval_score_routes_coverage(C.byref(e), C.c_void_p(ptr_of(near)), ld,
                                                                C.c_void_p(ptr_of(o32[3 * N:])), stream())
            else:
                entry = 'sf_eval_score_routes'
                status = _lib.lib.sf_eval_score_routes(C.byref(e), C.c_void_p(ptr_of(o32[3 * N:])), stream())
            if status == _lib.SF_ERR_UNSUPPORTED:             # a gold path above the kernel's 64 nodes
                self.fallbacks += 1
                return None
            _lib.check(status, entry)
            h64 = torch.empty(5, N, dtype=torch.float64).pin_memory()
            h32 = torch.empty(3 * N + 1, dtype=torch.int32).pin_memory()
            h64.copy_(o64, non_blocking=True)
            h32.copy_(o32, non_blocking=True)
            if self.coverage_metrics:
                hnear = torch.empty(N, ld, dtype=torch.float64).pin_memory()
                hnear.copy_(near, non_blocking=True)
            torch.cuda.current_stream().synchronize()         # the one host sync of the batch
        self.last_host_syncs = 1
        self.host_syncs += 1
        if int(h32[3 * N]):
            raise RuntimeError('%s: a route left its scan or does not start where its gold path does' % entry)
        f, k = h64.numpy(), h32.numpy()[:3 * N].reshape(3, N)
        margin = self.error_margin
        six = [EvalResult(a, b, c, d, bool(s), bool(o)) for a, b, c, d, s, o in
               zip(f[0].tolist(), f[1].tolist(), k[0].tolist(), f[2].tolist(), k[1].tolist(), k[2].tolist())]
        if not self.path_metrics:
            return six
        full = [path_metrics_of(r, sh, dtw, len(gt['path']), margin)
                for r, sh, dtw, (gt, _) in zip(six, f[3].tolist(), f[4].tolist(), routes)]
        if not self.coverage_metrics:
            return full
        lengths = self._gold_lengths()
        return [coverage_metrics_of(r, row[:len(gt['path'])], lengths[gt['path_id']], margin)
                for r, row, (gt, _) in zip(full, hnear.numpy().tolist(), routes)]

    def score_routes(self, instr_ids, trajectories):
        """What `_score_item(instr_id, trajectory)` returns for every pair, as one batch: EvalResult -- PathEvalResult
        with path_metrics, CoverageEvalResult with coverage_metrics -- per route (a trajectory: [(viewpoint, heading,
        elevation), ...] or a result of a device rollout)."""
        return self._score_routes([self._route_of(i, p) for i, p in zip(instr_ids, trajectories)])

    # ---- eval.py:86-145
    def score_results(self, results):
        """results: instr_id -> dictionary with (at least) 'trajectory' -- or a result of a device rollout
        (nav._Trajectory), which is scored from its nav rows."""
        self.scores = defaultdict(list)
        model_scores = []
        instr_ids = set(self.instr_ids)
        taken, on_device = [], []
        for instr_id, result in results.items():
            if instr_id in instr_ids:
                instr_ids.remove(instr_id)
                if self.path_metrics:                        # every result of the batch in one launch (or the host loop)
                    taken.append(self._route_of(instr_id, result if hasattr(result, 'nav_rows') else result['trajectory']))
                elif hasattr(result, 'nav_rows'):
                    on_device.append((instr_id, result))
                    taken.append(None)
                else:
                    taken.append(self._score_item(instr_id, result['trajectory']))
                if 'score' in result:
                    model_scores.append(result['score'])
        if self.path_metrics:
            taken = self._score_routes(taken)
        if on_device:
            scored = iter(self._score_device_results(on_device))
            taken = [next(scored) if r is None else r for r in taken]
        for r in taken:
            for name, v in zip(_LISTS, (r.nav_error, r.oracle_error, r.trajectory_steps, r.trajectory_length,
                                        r.success, r.oracle_success)):
                self.scores[name].append(v)
            if self.path_metrics:
                for name, v in zip(_PATH_LISTS, r[6:11]):
                    self.scores[name].append(v)
            if self.coverage_metrics:
                for name, v in zip(_COVERAGE_LISTS, r[11:]):
                    self.scores[name].append(v)
        return self._summary(instr_ids, len(taken), model_scores), self.scores

    def _summary(self, missing, instr_count, model_scores):
        assert len(missing) == 0, 'Missing %d of %d instruction ids from %s' % (
            len(missing), len(self.instr_ids), ','.join(self.splits))
        sc = self.scores
        assert len(sc['nav_errors']) == len(self.instr_ids)
        summary = {
            'nav_error': np.average(sc['nav_errors']),
            'oracle_error': np.average(sc['oracle_errors']),
            'steps': np.average(sc['trajectory_steps']),
            'lengths': np.average(sc['trajectory_lengths']),
            'success_rate': float(sum(sc['success']) / len(sc['success'])),
            'oracle_rate': float(sum(sc['oracle_success']) / len(sc['oracle_success'])),
        }
        if len(model_scores) > 0:
            assert len(model_scores) == instr_count
            summary['model_score'] = np.average(model_scores)
        if self.path_metrics:
            for name in ('spl', 'ndtw', 'sdtw'):
                summary[name] = np.average(sc[name])
        if self.coverage_metrics:
            summary['cls'] = np.average(sc['cls'])
        return summary

    def score_file(self, output_file):
        with open(output_file) as f:
            return self.score_results(json.load(f))

    # ---- agent.test() + score_results as one device sweep
    def _sweepable(self, agent, use_dropout, feedback):
        """The navigation table to sweep on -- or None where `Seq2SeqAgent._rollout_on_graph` would not take the agent
        (a process group, no device table, test_graph = False, feedback other than argmax, dropout on) or the
        distances are not on the device."""
        if feedback != 'argmax' or use_dropout or not getattr(agent, 'test_graph', False):
            return None
        nav = agent._device_table() if hasattr(agent, '_device_table') else None
        if nav is None or agent._engine is None or agent._engine.group is not None or self.table.dev is None:
            return None
        from . import _lib                                   # (loaded: the distances are on the device)
        if self.path_metrics and not 1 <= self._gold_table()['longest'] <= _lib.SF_EVAL_MAX_GOLD:
            return None                                      # (sf_eval_score_routes would refuse: one lane per gold node)
        return nav

    def _by_test(self, agent, use_dropout, feedback):
        self.fallbacks += 1
        agent.test(use_dropout=use_dropout, feedback=feedback)
        return self.score_results(agent.results)

    def _buffers(self, dev, K, S, B, keep):
        """Device arrays and pinned mirrors of a sweep of at most K minibatches, kept between sweeps (a sweep ends with
        a host sync: nothing of the previous one is in flight when the next one writes them)."""
        import torch
        key = (str(dev), K, S, B, len(self.instr_ids))
        buf = self._sweep_buffers.get(key)
        if buf is None:
            n = len(self.instr_ids)
            d = lambda *s, dt: torch.empty(*s, dtype=dt, device=dev)                      # noqa: E731
            p = lambda *s, dt: torch.empty(*s, dtype=dt).pin_memory()                     # noqa: E731
            i32, i64, f32, f64 = torch.int32, torch.int64, torch.float32, torch.float64
            w32, w64 = (5, 5) if self.path_metrics else (4, 3)                            # (+ gold_id; + shortest, dtw)
            buf = dict(per32=d(K, w32, B, dt=i32), per64=d(K, B, dt=i64), per32_h=p(K, w32, B, dt=i32),
                       per64_h=p(K, B, dt=i64),
                       out64=d(w64, n, dt=f64), out32=d(3, n, dt=i32), out64_h=p(w64, n, dt=f64), out32_h=p(3, n, dt=i32),
                       loss=d(K, dt=f32), loss_h=p(K, dt=f32), sc=d(K, S, B, dt=f32), sc_h=p(K, S, B, dt=f32),
                       err=d(1, dt=i32), err_h=p(1, dt=i32))
            if self.path_metrics:
                buf['first'] = torch.arange(B, dtype=i64, device=dev)                     # sweep layout: row_first[b] = b
            if self.coverage_metrics:                                                     # near [slot, gold position]
                ld = self._gold_table()['longest']
                buf.update(near=d(n, ld, dt=f64), near_h=p(n, ld, dt=f64))
            self._sweep_buffers = {key: buf}
        if keep and 'rows_h' not in buf:
            import torch
            p = lambda *s, dt: torch.empty(*s, dtype=dt).pin_memory()                     # noqa: E731
            buf.update(rows_h=p(K, S + 1, B, dt=torch.int32), views_h=p(K, S + 1, B, dt=torch.int32),
                       acts_h=p(K, S, B, dt=torch.int64))
        return buf

    def score_agent(self, agent, use_dropout=False, feedback='argmax', keep_results=False):
        """What `agent.test(use_dropout, feedback)` followed by `score_results(agent.results)` returns, as ONE sweep on
        the device: the environment is walked exactly as BaseAgent.test walks it (reset_epoch, reset(sort=True) until an
        id repeats, the first occurrence of an id wins -- `env.ix` and `random` end where test() leaves them), every
        minibatch's captured rollout is replayed back to back with sf_eval_score behind it on the same stream (ids
        already issued, and ids outside `instr_ids`, write nothing), and the host waits ONCE, after the last minibatch
        (`last_host_syncs`; the capture of a rollout nobody has captured yet synchronises on its own).  `agent.losses`
        is set as test() sets it; `agent.results` stays empty unless keep_results (the row / view / action downloads per
        minibatch, still without a wait in between).  A raised fault word, or an agent `_rollout_on_graph` does not
        take, means agent.test() + score_results instead (`fallbacks`): a faulting sweep is never scored, and the
        environment's item order and `random` are put back first, so that test() walks what the sweep walked.
        With path_metrics the launch behind every rollout is sf_eval_score_routes in its sweep layout (the same arrays,
        plus the episode's gold path index): still one host sync.  With coverage_metrics it is
        sf_eval_score_routes_coverage, which also fills `near` [instruction, gold position]: one more download behind the
        same sync."""
        if hasattr(agent, 'walk_policy'):                     # a baseline agent: its own sweep, or its own test()
            return self._score_table_agent(agent, keep_results)
        nav = self._sweepable(agent, use_dropout, feedback)
        if nav is None:
            return self._by_test(agent, use_dropout, feedback)
        import torch
        from . import _lib
        from .nav import DeviceNavBatch
        from .runtime import stream, fault_views, take_fault, WeightsMoved
        env, eng, t = agent.env, agent._engine, self.table
        dev = agent._device()
        agent.feedback = feedback
        for mod in (agent.encoder, agent.decoder):
            mod.eval()
        agent.set_beam_size(1)
        agent.__dict__.pop('_rollout_inflight', None)         # (nothing issued ahead by an earlier loop is ours)
        S, B = agent.episode_len, min(env.batch_size, max(1, len(env.data)))
        K = -(-len(env.data) // B) + 1                        # an id repeats in minibatch ceil(N / B) + 1 at the latest
        buf = self._buffers(dev, K, S, B, keep_results)
        gold = self._gold_table() if self.path_metrics else None
        per32, per64 = buf['per32_h'].numpy(), buf['per64_h'].numpy()
        walk0 = (list(env.data), random.getstate())          # (a faulting sweep is undone: test() then walks from here)
        env.reset_epoch()
        agent.losses, agent.results = [], {}
        syncs = 0
        for w in fault_views(dev):                            # (whatever an earlier pass left behind is not ours)
            w.zero_()
        buf['err'].zero_()
        order, where, seen, issued, looped = [], [], set(), [], False
        ptr_of = lambda x: x.data_ptr()                       # noqa: E731
        with torch.no_grad():
            while not looped:
                env.reset(sort=True)
                items = list(env.batch)
                k = len(issued)
                if len(items) != B or k >= K:
                    raise RuntimeError('score_agent: minibatch %d holds %d items (batches of %d, at most %d)'
                                       % (k, len(items), B, K))
                for b, it in enumerate(items):
                    iid, scan = it['instr_id'], it['scan']
                    slot = -1
                    if iid in seen:
                        looped = True
                    else:
                        seen.add(iid)
                        if iid in self.instr_ids:
                            slot = len(order)
                            order.append(iid)
                            where.append((k, b))
                    goal = self.gt.get(it.get('path_id'), it)['path'][-1]
                    per32[k, 0, b], per32[k, 1, b] = nav.row_of[(scan, goal)], self._local_rows(nav, scan)
                    per32[k, 2, b], per32[k, 3, b] = t.m[scan], slot
                    per64[k, b] = t.off[scan]
                    if gold is not None:
                        per32[k, 4, b] = gold['ids'].get(it.get('path_id'), 0)            # (read only where slot >= 0)
                host = DeviceNavBatch.host_arrays_for(nav, items, agent.max_instruction_length,
                                                      agent.reverse_instruction, True)
                key = agent._test_graph_key(nav, eng, B)
                for attempt in (0, 1):
                    cached = agent.__dict__.setdefault('_test_graphs', {}).get(key)
                    if cached is None:
                        cached = agent._capture_test_rollout(nav, items, key, host)
                    else:
                        mirrors = cached[2].__dict__.setdefault('_sweep_mirrors', [])
                        while len(mirrors) <= k:
                            mirrors.append(cached[2].new_mirror())
                        cached[2].load(items, host, mirror=mirrors[k])
                    try:
                        cached[0]()
                        break
                    except WeightsMoved:                      # (a weight moved since the capture: capture again)
                        if attempt:
                            raise
                        agent._test_graphs.pop(key, None)
                st, batch = cached[1], cached[2]
                buf['per32'][k].copy_(buf['per32_h'][k], non_blocking=True)
                buf['per64'][k].copy_(buf['per64_h'][k], non_blocking=True)
                d32, o64, o32 = buf['per32'][k], buf['out64'], buf['out32']
                if gold is not None:                          # the sweep layout of sf_eval_score_routes: + shortest, dtw
                    ep = _lib.EvalRoutes(S, B, len(self.instr_ids), B, len(gold['ids']), len(gold['node']),
                                         gold['longest'], 0, (S + 1) * B, ptr_of(batch.row), ptr_of(buf['first']), None,
                                         ptr_of(st.actions), ptr_of(gold['dev'][0]), ptr_of(gold['dev'][1]),
                                         ptr_of(d32[4]), ptr_of(d32[1]), ptr_of(d32[2]), ptr_of(buf['per64'][k]),
                                         ptr_of(d32[3]), ptr_of(t.dev), self.error_margin,
                                         *[ptr_of(o64[i]) for i in (0, 1, 2, 3, 4)], *[ptr_of(o32[i]) for i in (0, 1, 2)])
                    if self.coverage_metrics:
                        _lib.call('sf_eval_score_routes_coverage', C.byref(ep), C.c_void_p(ptr_of(buf['near'])),
                                  gold['longest'], C.c_void_p(buf['err'].data_ptr()), stream())
                    else:
                        _lib.call('sf_eval_score_routes', C.byref(ep), C.c_void_p(buf['err'].data_ptr()), stream())
                else:
                    ep = _lib.EvalEpisodes(S, B, len(self.instr_ids), 0, ptr_of(batch.row), ptr_of(st.actions),
                                           ptr_of(d32[0]), ptr_of(d32[1]), ptr_of(d32[2]), ptr_of(buf['per64'][k]),
                                           ptr_of(d32[3]), ptr_of(t.dev), self.error_margin, ptr_of(o64[0]),
                                           ptr_of(o64[1]), ptr_of(o64[2]), ptr_of(o32[0]), ptr_of(o32[1]), ptr_of(o32[2]))
                    _lib.call('sf_eval_score', C.byref(ep), C.c_void_p(buf['err'].data_ptr()), stream())
                buf['loss'][k:k + 1].copy_(st.loss_buf.reshape(1))
                buf['sc'][k].copy_(st.step_scores[:S])
                if keep_results:
                    buf['rows_h'][k].copy_(batch.row[:S + 1], non_blocking=True)
                    buf['views_h'][k].copy_(batch.view[:S + 1], non_blocking=True)
                    buf['acts_h'][k].copy_(st.actions[:S], non_blocking=True)
                issued.append(items)
            n_mb = len(issued)
            for name in ('out64', 'out32', 'loss', 'sc', 'err') + (('near',) if self.coverage_metrics else ()):
                buf[name + '_h'].copy_(buf[name], non_blocking=True)
            faults = fault_views(dev)
            fpin = torch.empty(len(faults), dtype=torch.int32).pin_memory()
            fpin.copy_(torch.cat(faults) if len(faults) > 1 else faults[0], non_blocking=True)
            torch.cuda.current_stream().synchronize()         # the one host sync of the sweep
            syncs += 1
        self.sweeps += 1
        if any(fpin.tolist()):
            take_fault(dev)                                   # (read and cleared: test() starts clean)
            self.last_host_syncs = syncs + 1
            self.host_syncs += syncs + 1
            env.data[:] = walk0[0]
            random.setstate(walk0[1])
            return self._by_test(agent, use_dropout, feedback)
        self.last_host_syncs = syncs
        self.host_syncs += syncs
        if int(buf['err_h'][0]):
            raise RuntimeError('%s: a rollout left its scan, or a slot its array'
                               % ('sf_eval_score_routes_coverage' if self.coverage_metrics else
                                  'sf_eval_score_routes' if self.path_metrics else 'sf_eval_score'))
        M = len(order)
        o64, o32 = buf['out64_h'].numpy(), buf['out32_h'].numpy()
        self._scores_of_sweep(order, o64, o32, buf['near_h'].numpy() if self.coverage_metrics else None)
        # 'score' of a result: the sequential float32 sum of its step scores up to the stop (nav.trajectories_from)
        sc = buf['sc_h'].numpy()[:n_mb]
        totals = np.cumsum(sc, axis=1, dtype=np.float32)
        kb = np.asarray(where, np.int64).reshape(M, 2)
        model_scores = totals[kb[:, 0], o32[0, :M] - 1, kb[:, 1]].tolist()
        agent.losses = buf['loss_h'][:n_mb].tolist()
        agent.loss = torch.tensor(agent.losses[-1])
        if keep_results:
            for k, items in enumerate(issued):
                rows, views, acts = (buf[x][k].numpy().copy() for x in ('rows_h', 'views_h', 'acts_h'))
                for tr, it in zip(cached[2].trajectories_from(items, S, rows, views, acts, sc[k].copy()), items):
                    tr['instr_encoding'] = it['instr_encoding']
                    agent.results.setdefault(tr['instr_id'], tr)
        return self._summary(self.instr_ids - set(order), M, model_scores), self.scores

    def _scores_of_sweep(self, order, o64, o32, near):
        """`self.scores` from a sweep's downloaded outputs: o64 [3 or 5, n_slots] (nav_error, oracle_error, length,
        + shortest, dtw), o32 [3, n_slots] (steps, success, oracle_success), near [n_slots, longest] with
        coverage_metrics; slot i belongs to instruction order[i]."""
        M = len(order)
        self.scores = defaultdict(list)
        self.scores['nav_errors'] = o64[0, :M].tolist()
        self.scores['oracle_errors'] = o64[1, :M].tolist()
        self.scores['trajectory_steps'] = o32[0, :M].tolist()
        self.scores['trajectory_lengths'] = o64[2, :M].tolist()
        self.scores['success'] = (o32[1, :M] != 0).tolist()
        self.scores['oracle_success'] = (o32[2, :M] != 0).tolist()
        if self.path_metrics:                                 # spl, ndtw, sdtw per item by the one function of the host path
            lists = [self.scores[name] for name in _LISTS]
            goldn = [len(self.gt[int(iid.split('_')[0])]['path']) for iid in order]
            full = [path_metrics_of(EvalResult(*six), sh, dtw, g, self.error_margin)
                    for six, sh, dtw, g in zip(zip(*lists), o64[3, :M].tolist(), o64[4, :M].tolist(), goldn)]
            for i, name in enumerate(_PATH_LISTS):
                self.scores[name] = [r[6 + i] for r in full]
            if self.coverage_metrics:                         # cls per item by the one function of the host path
                lengths = self._gold_lengths()
                full = [coverage_metrics_of(r, row[:g], lengths[int(iid.split('_')[0])], self.error_margin)
                        for r, row, g, iid in zip(full, near[:M].tolist(), goldn, order)]
                for i, name in enumerate(_COVERAGE_LISTS):
                    self.scores[name] = [r[11 + i] for r in full]

    # ---- a baseline agent's test() + score_results: one walk launch, one scoring launch
    def _score_table_agent(self, agent, keep_results=False):
        """score_agent for agents.StopAgent / ShortestAgent / RandomAgent.  The environment is walked as BaseAgent.test
        walks it (reset_epoch, reset() until an id repeats; `env.ix`, `random` and `np.random` end where test() leaves
        them: RandomAgent draws for every row of every minibatch, repeated ids included), but nothing is launched per
        minibatch: the first occurrences of the whole split are ONE sf_nav_walk launch, and behind it ONE
        sf_eval_score_routes launch over the walk's own arrays (row_stride = B, row_first[b] = b, the walk's n_steps;
        sf_eval_score_routes_coverage with coverage_metrics), then one host sync.  The classic six come from that
        launch whatever the metric switches say.  An agent without a table on the device, distances that are not
        there, or gold paths the kernel refuses: agent.test() + score_results (`fallbacks`)."""
        from . import _lib                                   # (loaded: the agent's class reads its policy from it)
        nav = agent._device_table()
        gold = self._gold_table() if nav is not None and self.table.dev is not None else None
        if gold is None or gold['dev'] is None or not 1 <= gold['longest'] <= _lib.SF_EVAL_MAX_GOLD:
            self.fallbacks += 1
            agent.test()
            return self.score_results(agent.results)
        import torch
        from .runtime import stream
        env, t = agent.env, self.table
        dev = t.dev.device
        env.reset_epoch()
        agent.losses, agent.results = [], {}
        walked, seen, looped = [], set(), False               # walked: (item, row, view, first action) per first occurrence
        while not looped:
            env.reset()
            items = list(env.batch)
            rows, views = nav.start_states(items)
            first = agent._first_actions(nav, rows, views)
            for b, it in enumerate(items):
                if it['instr_id'] in seen:
                    looped = True
                else:
                    seen.add(it['instr_id'])
                    walked.append((it, rows[b], views[b], 0 if first is None else first[b]))
        S, B, n = agent.walk_steps, len(walked), len(self.instr_ids)
        order = []
        i32 = np.zeros((4, B), np.int32)                      # gold_id, scan_base, m, slot
        i64 = np.zeros((2, B), np.int64)                      # row_first, dist_off
        i64[0] = np.arange(B)
        for b, (it, _, _, _) in enumerate(walked):
            scan, slot = it['scan'], -1
            if it['instr_id'] in self.instr_ids:
                slot = len(order)
                order.append(it['instr_id'])
            i32[:, b] = gold['ids'].get(it.get('path_id'), 0), self._local_rows(nav, scan), t.m[scan], slot
            i64[1, b] = t.off[scan]
        items = [w[0] for w in walked]
        hop, base = nav.hop_rows(items) if agent.walk_policy == _lib.SF_WALK_SHORTEST else (None, None)
        ptr_of = lambda x: x.data_ptr()                       # noqa: E731
        with torch.cuda.device(dev):
            out = nav.walk(agent.walk_policy, S, np.array([w[1] for w in walked], np.int32),
                           np.array([w[2] for w in walked], np.int32),
                           None if first is None else np.array([w[3] for w in walked], np.int32), hop, base)
            d32, d64 = torch.from_numpy(i32).to(dev), torch.from_numpy(i64).to(dev)
            o64 = torch.empty(5, n, dtype=torch.float64, device=dev)
            o32 = torch.zeros(3 * n + 1, dtype=torch.int32, device=dev)                   # (the last word: err)
            e = _lib.EvalRoutes(S, B, n, B, len(gold['ids']), len(gold['node']), gold['longest'], 0, (S + 1) * B,
                                ptr_of(out['row']), ptr_of(d64[0]), ptr_of(out['n_steps']), ptr_of(out['actions']),
                                ptr_of(gold['dev'][0]), ptr_of(gold['dev'][1]), ptr_of(d32[0]), ptr_of(d32[1]),
                                ptr_of(d32[2]), ptr_of(d64[1]), ptr_of(d32[3]), ptr_of(t.dev), self.error_margin,
                                *[ptr_of(o64[k]) for k in range(5)], *[ptr_of(o32[k * n:]) for k in range(3)])
            near = None
            if self.coverage_metrics:
                entry, ld = 'sf_eval_score_routes_coverage', gold['longest']
                near = torch.empty(n, ld, dtype=torch.float64, device=dev)
                _lib.call(entry, C.byref(e), C.c_void_p(ptr_of(near)), ld, C.c_void_p(ptr_of(o32[3 * n:])), stream())
            else:
                entry = 'sf_eval_score_routes'
                _lib.call(entry, C.byref(e), C.c_void_p(ptr_of(o32[3 * n:])), stream())
            down = [o64, o32, out['err']] + ([near] if near is not None else [])
            if keep_results:
                down += [out['row'], out['view'], out['n_steps']]
            got = [torch.empty(x.shape, dtype=x.dtype).pin_memory() for x in down]
            for h, x in zip(got, down):
                h.copy_(x, non_blocking=True)
            torch.cuda.current_stream().synchronize()         # the one host sync of the sweep
        self.sweeps += 1
        self.last_host_syncs = 1
        self.host_syncs += 1
        if int(got[2][0]):
            raise agent.walk_error()
        if int(got[1][3 * n]):
            raise RuntimeError('%s: a walk left its scan, or a slot its array' % entry)
        self._scores_of_sweep(order, got[0].numpy(), got[1].numpy()[:3 * n].reshape(3, n),
                              got[3].numpy() if near is not None else None)
        if keep_results:
            rows, views, steps = (x.numpy() for x in got[-3:])
            for r in nav.walk_results(items, rows, views, steps):
                agent.results[r['instr_id']] = r
        return self._summary(self.instr_ids - set(order), len(order), []), self.scores


def evaluate_simple_agents(env, ev, result_dir, agent_types=('Stop', 'Shortest', 'Random')):
    """eval.py:155-163 for one environment and its evaluator: every baseline agent is tested, its results written to
    `<result_dir><split>_<type in lower case>_agent.json` and that file scored; the name and the summary are printed.
    Returns {type: summary}."""
    import pprint
    from .agents import BaseAgent
    split = ','.join(getattr(env, 'splits', None) or ev.splits)
    summaries = {}
    for agent_type in agent_types:
        outfile = '%s%s_%s_agent.json' % (result_dir, split, agent_type.lower())
        agent = BaseAgent.get_agent(agent_type)(env, outfile)
        agent.test()
        agent.write_results()
        summaries[agent_type], _ = ev.score_file(outfile)
        print('\n%s' % agent_type)
        pprint.PrettyPrinter(indent=4).pprint(summaries[agent_type])
    return summaries


def eval_simple_agents(args):
    """eval.py:148-163: the Stop / Shortest / Random table of every split, over compat.env's construction surface.  The
    result directory is train.RESULT_DIR when `train` imports (the reference's script beside the caller), else
    tasks/R2R/results/."""
    from .compat.env import ImageFeatures, R2RBatch
    try:
        import train
        result_dir = train.RESULT_DIR
    except ImportError:
        result_dir = 'tasks/R2R/results/'
    img_features = ImageFeatures.from_args(args)
    out = {}
    for split in ['train', 'val_seen', 'val_unseen', 'test']:
        env = R2RBatch(img_features, batch_size=1, splits=[split])
        out[split] = evaluate_simple_agents(env, Evaluation([split]), result_dir)
    return out
