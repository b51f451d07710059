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


def _err_text(entry, noun, ragged=False):
    """The sentence for a raised err word of a scoring launch over `noun`s (include/sf_hip.h: the refusals per route)."""
    return '%s: a %s left its scan%s' % (entry, noun, ' or does not start where its gold path does' if ragged
                                         else ', or a slot its array')


class _Outputs:
    """The output block of a scoring launch over n slots, with a pinned mirror (`*_h`) of every array:
      o64 [5, n]   nav_error, oracle_error, length, shortest, dtw ([3, n] with wide=False: sf_eval_score's)
      o32 [3, n]   steps, success, oracle_success
      err [1]      only ever raised by the kernels: zeroed here, and by an owner that keeps the block, before it launches
      near [n, near_ld]   with near_ld > 0: the coverage launch's least distance to every gold node
    `download()` issues the copies to the mirrors on the current stream; behind the caller's sync, `check(text)` raises
    a set err word in the words the launch gave and `host()` is (o64, o32, near or None) as numpy arrays."""

    def __init__(self, dev, n, wide=True, near_ld=0):
        import torch
        pair = lambda shape, dt: (torch.empty(shape, dtype=dt, device=dev),           # noqa: E731
                                  torch.empty(shape, dtype=dt).pin_memory())
        self.o64, self.o64_h = pair((5 if wide else 3, n), torch.float64)
        self.o32, self.o32_h = pair((3, n), torch.int32)
        self.err, self.err_h = pair((1,), torch.int32)
        self.near, self.near_h = pair((n, near_ld), torch.float64) if near_ld else (None, None)
        self.err.zero_()

    def download(self):
        for name in ('o64', 'o32', 'err') + (('near',) if self.near is not None else ()):
            getattr(self, name + '_h').copy_(getattr(self, name), non_blocking=True)

    def check(self, text):
        if int(self.err_h[0]):
            raise RuntimeError(text)

    def host(self):
        return self.o64_h.numpy(), self.o32_h.numpy(), None if self.near is None else self.near_h.numpy()


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
        cost = D[np.ix_(rows, gold)].tolist()
        r = path_metrics_of(r, float(D[rows[0], goal]), dtw_rows(cost), len(gold), self.error_margin)
        if not self.coverage_metrics:
            return r
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

    def _episode_words(self, nav, items, slots):
        """int64 [5, B]: gold_id, scan_base, m, dist_off, slot -- the per-episode words of a scoring launch, for items
        of the environment whose poses are rows of `nav`, or (nav = None) ground truths whose poses are local already.
        gold_id is 0 where the gold table has not been built (path_metrics off) or does not hold the item's path: the
        kernels read it only where slot >= 0."""
        t, ids = self.table, {} if self._gold is None else self._gold['ids']
        return np.array([(ids.get(it.get('path_id'), 0), 0 if nav is None else self._local_rows(nav, it['scan']),
                          t.m[it['scan']], t.off[it['scan']], slot)
                         for it, slot in zip(items, slots)], np.int64).reshape(len(items), 5).T

    def _launch_route_scoring(self, out, noun, *, S, B, n_slots, row_stride, n_rows, row, row_first, gold_id,
                              scan_base, m, dist_off, slot, n_steps=None, actions=None, refusable=False):
        """THE route-scoring launch (include/sf_hip.h: sf_eval_routes), issued on the current stream for B routes
        (device tensors, by name) into the output block `out`: sf_eval_score_routes_coverage with coverage_metrics
        -- it also fills out.near -- else sf_eval_score_routes.  The gold paths, the distances and the margin are the
        evaluator's.  The layouts:
          ragged   routes back to back in `row`: row_stride = 1, row_first = their offsets, n_steps given (S = 0)
          sweep    row [S+1, B] as a rollout or a walk leaves it: row_stride = B, row_first[b] = b, and either `actions`
                   [S, B] (the step count is derived from them) or the walk's own n_steps
        Returns (status, text): `text` is the sentence for a raised err word in the caller's terms (`noun`: 'route',
        'rollout', 'walk'), for `out.check(text)` after the caller's sync.  A failing status raises here; only a
        `refusable` caller gets SF_ERR_UNSUPPORTED back (a gold path above SF_EVAL_MAX_GOLD nodes, nothing launched)."""
        from . import _lib
        from .runtime import stream
        gold = self._gold_table()
        at = lambda x: None if x is None else x.data_ptr()    # noqa: E731
        e = _lib.EvalRoutes(S=S, B=B, n_slots=n_slots, row_stride=row_stride, n_gold=len(gold['ids']),
                            n_gold_nodes=len(gold['node']), max_gold=gold['longest'], n_rows=n_rows, row=at(row),
                            row_first=at(row_first), n_steps=at(n_steps), actions=at(actions),
                            gold_off=at(gold['dev'][0]), gold_node=at(gold['dev'][1]), gold_id=at(gold_id),
                            scan_base=at(scan_base), m=at(m), dist_off=at(dist_off), slot=at(slot),
                            table=at(self.table.dev), margin=self.error_margin,
                            nav_error=at(out.o64[0]), oracle_error=at(out.o64[1]), length=at(out.o64[2]),
                            shortest=at(out.o64[3]), dtw=at(out.o64[4]),
                            steps=at(out.o32[0]), success=at(out.o32[1]), oracle_success=at(out.o32[2]))
        if self.coverage_metrics:
            entry, near = 'sf_eval_score_routes_coverage', (C.c_void_p(at(out.near)), out.near.shape[1])
        else:
            entry, near = 'sf_eval_score_routes', ()
        status = getattr(_lib.lib, entry)(C.byref(e), *near, C.c_void_p(at(out.err)), stream())
        if not (refusable and status == _lib.SF_ERR_UNSUPPORTED):
            _lib.check(status, entry)
        return status, _err_text(entry, noun, ragged=row_stride == 1)

    def _assemble(self, gts, o64, o32, near=None, lists=False):
        """A scoring launch's downloaded outputs (_Outputs.host()) -> the per-item results of this evaluator's type, or
        with `lists` -> `self.scores`, one list per field.  Slot i belongs to ground truth gts[i]; slots behind the last
        one, and the elements of a `near` row behind its gold path, hold nothing.  The classic six come by columns (and
        stay columns where nothing else is asked for); spl / ndtw / sdtw and coverage / length_score / cls are formed
        per item by the one function each that the host path uses."""
        M = len(gts)
        cols = (o64[0, :M].tolist(), o64[1, :M].tolist(), o32[0, :M].tolist(), o64[2, :M].tolist(),
                (o32[1, :M] != 0).tolist(), (o32[2, :M] != 0).tolist())
        if self.path_metrics or not lists:
            out = [EvalResult(*r) for r in zip(*cols)]
            margin = self.error_margin
            if self.path_metrics:
                out = [path_metrics_of(r, sh, dtw, len(gt['path']), margin)
                       for r, sh, dtw, gt in zip(out, o64[3, :M].tolist(), o64[4, :M].tolist(), gts)]
            if self.coverage_metrics:
                lengths = self._gold_lengths()
                out = [coverage_metrics_of(r, row[:len(gt['path'])], lengths[gt['path_id']], margin)
                       for r, row, gt in zip(out, near[:M].tolist(), gts)]
            if not lists:
                return out
            cols = zip(*out)
        return self._scores_of(cols)

    def _scores_of(self, cols):
        """`self.scores` from the columns of the results: one list per field of this evaluator's result type."""
        names = _LISTS + (_PATH_LISTS if self.path_metrics else ()) + (_COVERAGE_LISTS if self.coverage_metrics else ())
        self.scores = defaultdict(list, zip(names, map(list, cols)))
        return self.scores

    def _score_routes_on_device(self, routes):
        import torch
        from . import _lib
        t, gold = self.table, self._gold_table()
        if gold['dev'] is None:
            return None
        dev = t.dev.device
        N = len(routes)
        n = np.array([len(rows) - 1 for _, rows in routes], np.int64)
        first = np.concatenate(([0], np.cumsum(n[:-1] + 1)))
        w = self._episode_words(None, [gt for gt, _ in routes], range(N))
        i32 = np.concatenate((w[[0, 1, 2, 4]], n[None])).astype(np.int32)      # gold_id, scan_base, m, slot, n_steps
        i64 = np.stack((first, w[3]))                                          # row_first, dist_off
        poses = np.concatenate([rows for _, rows in routes]).astype(np.int32)
        with torch.cuda.device(dev):
            d32, d64, rows_d = (torch.from_numpy(a).to(dev) for a in (i32, i64, poses))
            out = _Outputs(dev, N, near_ld=gold['longest'] if self.coverage_metrics else 0)
            status, text = self._launch_route_scoring(out, 'route', S=0, B=N, n_slots=N, row_stride=1,
                                                      n_rows=len(poses), row=rows_d, row_first=d64[0], n_steps=d32[4],
                                                      gold_id=d32[0], scan_base=d32[1], m=d32[2], dist_off=d64[1],
                                                      slot=d32[3], refusable=True)
            if status == _lib.SF_ERR_UNSUPPORTED:             # a gold path above the kernel's 64 nodes
                self.fallbacks += 1
                return None
            out.download()
            torch.cuda.current_stream().synchronize()         # the one host sync of the batch
        self.last_host_syncs = 1
        self.host_syncs += 1
        out.check(text)
        return self._assemble([gt for gt, _ in routes], *out.host())

    def score_routes(self, instr_ids, trajectories):
        """What `_score_item(instr_id, trajectory)` returns for every pair, as one batch: EvalResult -- PathEvalResult
        with path_metrics, CoverageEvalResult with coverage_metrics -- per route (a trajectory: [(viewpoint, heading,
        elevation), ...] or a result of a device rollout)."""
        return self._score_routes([self._route_of(i, p) for i, p in zip(instr_ids, trajectories)])

    # ---- eval.py:86-145
    def score_results(self, results):
        """results: instr_id -> dictionary with (at least) 'trajectory' -- or a result of a device rollout
        (nav._Trajectory), which is scored from its nav rows."""
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
        self._scores_of(zip(*taken))
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
        p = lambda *s, dt: torch.empty(*s, dtype=dt).pin_memory()                         # noqa: E731
        if buf is None:
            d = lambda *s, dt: torch.empty(*s, dtype=dt, device=dev)                      # noqa: E731
            i32, i64, f32 = torch.int32, torch.int64, torch.float32
            w32 = 5 if self.path_metrics else 4                                           # (+ gold_id)
            buf = dict(per32=d(K, w32, B, dt=i32), per64=d(K, B, dt=i64), per32_h=p(K, w32, B, dt=i32),
                       per64_h=p(K, B, dt=i64),
                       out=_Outputs(dev, len(self.instr_ids), wide=self.path_metrics,      # near [slot, gold position]
                                    near_ld=self._gold_table()['longest'] if self.coverage_metrics else 0),
                       loss=d(K, dt=f32), loss_h=p(K, dt=f32), sc=d(K, S, B, dt=f32), sc_h=p(K, S, B, dt=f32))
            if self.path_metrics:
                buf['first'] = torch.arange(B, dtype=i64, device=dev)                     # sweep layout: row_first[b] = b
            self._sweep_buffers = {key: buf}
        if keep and 'rows_h' not in buf:
            buf.update(rows_h=p(K, S + 1, B, dt=torch.int32), views_h=p(K, S + 1, B, dt=torch.int32),
                       acts_h=p(K, S, B, dt=torch.int64))
        return buf

    def score_agent(self, agent, use_dropout=False, feedback='argmax', keep_results=False):
        """What `agent.test(use_dropout, feedback)` followed by `score_results(agent.results)` returns, as ONE sweep on
        the device.  The environment is walked exactly as BaseAgent.test walks it (sweeps.epoch_minibatches with
        reset(sort=True): `env.ix` and `random` end where test() leaves them), every minibatch's captured rollout is
        replayed back to back with the scoring launch behind it on the same stream -- sf_eval_score, or with
        path_metrics `_launch_route_scoring` in its sweep layout over the same arrays; ids already issued, and ids
        outside `instr_ids`, write nothing -- and the host waits ONCE, after the last minibatch (`last_host_syncs`; the
        capture of a rollout nobody has captured yet synchronises on its own).  `agent.losses` is set as test() sets it;
        `agent.results` stays empty unless keep_results (the row / view / action downloads per minibatch, still without
        a wait in between).  A raised fault word, or an agent `_rollout_on_graph` does not take, means agent.test() +
        score_results instead (`fallbacks`): a faulting sweep is never scored, and the environment's item order and
        `random` are put back first, so that test() walks what the sweep walked."""
        if hasattr(agent, 'walk_policy'):                     # a baseline agent: its own sweep, or its own test()
            return self._score_table_agent(agent, keep_results)
        nav = self._sweepable(agent, use_dropout, feedback)
        if nav is None:
            return self._by_test(agent, use_dropout, feedback)
        import torch
        from . import _lib
        from .runtime import stream, clear_faults, download_faults, take_fault
        from .sweeps import epoch_minibatches, snapshot, restore
        env, t = agent.env, self.table
        dev = agent._device()
        agent.feedback = feedback
        for mod in (agent.encoder, agent.decoder):
            mod.eval()
        agent.set_beam_size(1)
        agent.__dict__.pop('_rollout_inflight', None)         # (nothing issued ahead by an earlier loop is ours)
        S, B = agent.episode_len, min(env.batch_size, max(1, len(env.data)))
        K = -(-len(env.data) // B) + 1                        # an id repeats in minibatch ceil(N / B) + 1 at the latest
        buf = self._buffers(dev, K, S, B, keep_results)
        out = buf['out']
        if self.path_metrics:
            self._gold_table()                                # (the episodes' gold ids are read from it)
        per32, per64 = buf['per32_h'].numpy(), buf['per64_h'].numpy()
        walk0 = snapshot(env)                                 # (a faulting sweep is undone: test() then walks from here)
        env.reset_epoch()
        agent.losses, agent.results = [], {}
        clear_faults(dev)                                     # (whatever an earlier pass left behind is not ours)
        out.err.zero_()
        order, where, issued = [], [], []
        ptr_of = lambda x: x.data_ptr()                       # noqa: E731
        with torch.no_grad():
            for k, items, fresh in epoch_minibatches(env, sort=True):
                if len(items) != B or k >= K:
                    raise RuntimeError('score_agent: minibatch %d holds %d items (batches of %d, at most %d)'
                                       % (k, len(items), B, K))
                slots = [-1] * B
                for b, it in enumerate(items):
                    if fresh[b] and it['instr_id'] in self.instr_ids:
                        slots[b] = len(order)
                        order.append(it['instr_id'])
                        where.append((k, b))
                w = self._episode_words(nav, items, slots)
                per32[k, 0] = [nav.row_of[(it['scan'], self.gt.get(it.get('path_id'), it)['path'][-1])] for it in items]
                per32[k, 1:4], per64[k] = w[[1, 2, 4]], w[3]      # goal_row, scan_base, m, slot (+ gold_id); dist_off
                if self.path_metrics:
                    per32[k, 4] = w[0]
                st, batch = self._replay_rollout(agent, nav, items, k, B)
                buf['per32'][k].copy_(buf['per32_h'][k], non_blocking=True)
                buf['per64'][k].copy_(buf['per64_h'][k], non_blocking=True)
                d32 = buf['per32'][k]
                if self.path_metrics:
                    _, text = self._launch_route_scoring(out, 'rollout', S=S, B=B, n_slots=len(self.instr_ids),
                                                         row_stride=B, n_rows=(S + 1) * B, row=batch.row,
                                                         row_first=buf['first'], actions=st.actions, gold_id=d32[4],
                                                         scan_base=d32[1], m=d32[2], dist_off=buf['per64'][k], slot=d32[3])
                else:
                    text = _err_text('sf_eval_score', 'rollout')
                    ep = _lib.EvalEpisodes(S=S, B=B, n_slots=len(self.instr_ids), row=ptr_of(batch.row),
                                           actions=ptr_of(st.actions), goal_row=ptr_of(d32[0]), scan_base=ptr_of(d32[1]),
                                           m=ptr_of(d32[2]), dist_off=ptr_of(buf['per64'][k]), slot=ptr_of(d32[3]),
                                           table=ptr_of(t.dev), margin=self.error_margin,
                                           nav_error=ptr_of(out.o64[0]), oracle_error=ptr_of(out.o64[1]),
                                           length=ptr_of(out.o64[2]), steps=ptr_of(out.o32[0]),
                                           success=ptr_of(out.o32[1]), oracle_success=ptr_of(out.o32[2]))
                    _lib.call('sf_eval_score', C.byref(ep), C.c_void_p(ptr_of(out.err)), stream())
                buf['loss'][k:k + 1].copy_(st.loss_buf.reshape(1))
                buf['sc'][k].copy_(st.step_scores[:S])
                if keep_results:
                    buf['rows_h'][k].copy_(batch.row[:S + 1], non_blocking=True)
                    buf['views_h'][k].copy_(batch.view[:S + 1], non_blocking=True)
                    buf['acts_h'][k].copy_(st.actions[:S], non_blocking=True)
                issued.append(items)
            n_mb = len(issued)
            out.download()
            for name in ('loss', 'sc'):
                buf[name + '_h'].copy_(buf[name], non_blocking=True)
            fpin = download_faults(dev)
            torch.cuda.current_stream().synchronize()         # the one host sync of the sweep
        self.sweeps += 1
        if any(fpin.tolist()):
            take_fault(dev)                                   # (read and cleared: test() starts clean)
            self.last_host_syncs = 2
            self.host_syncs += 2
            restore(env, walk0)
            return self._by_test(agent, use_dropout, feedback)
        self.last_host_syncs = 1
        self.host_syncs += 1
        out.check(text)
        M = len(order)
        o64, o32, near = out.host()
        self._assemble([self.gt[int(iid.split('_')[0])] for iid in order], o64, o32, near, lists=True)
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
                for tr, it in zip(batch.trajectories_from(items, S, rows, views, acts, sc[k].copy()), items):
                    tr['instr_encoding'] = it['instr_encoding']
                    agent.results.setdefault(tr['instr_id'], tr)
        return self._summary(self.instr_ids - set(order), M, model_scores), self.scores

    @staticmethod
    def _replay_rollout(agent, nav, items, k, B):
        """Minibatch k of a sweep through the agent's captured test rollout: loaded through the k-th of the capture's
        staging mirrors (no wait for one in the middle of a sweep) and replayed -- or captured, where nobody has yet, or
        a weight moved since.  Returns (the rollout's state, its device batch)."""
        from .nav import DeviceNavBatch
        from .runtime import WeightsMoved
        host = DeviceNavBatch.host_arrays_for(nav, items, agent.max_instruction_length, agent.reverse_instruction, True)
        key = agent._test_graph_key(nav, agent._engine, B)
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
            except WeightsMoved:                              # (a weight moved since the capture: capture again)
                if attempt:
                    raise
                agent._test_graphs.pop(key, None)
        return cached[1], cached[2]

    # ---- a baseline agent's test() + score_results: one walk launch, one scoring launch
    def _score_table_agent(self, agent, keep_results=False):
        """score_agent for agents.StopAgent / ShortestAgent / RandomAgent.  The epoch is walked on the host with
        reset() (`np.random` too ends where test() leaves it: RandomAgent draws for every row of every minibatch,
        repeated ids included), but nothing is launched per minibatch: the first occurrences of the whole split are ONE
        sf_nav_walk launch, and behind it ONE `_launch_route_scoring` over the walk's own arrays and n_steps, then one
        host sync.  The classic six come from that launch whatever the metric switches say.  An agent without a table
        on the device, distances that are not there, or gold paths the kernel refuses: agent.test() + score_results
        (`fallbacks`)."""
        from . import _lib                                   # (loaded: the agent's class reads its policy from it)
        nav = agent._device_table()
        gold = self._gold_table() if nav is not None and self.table.dev is not None else None
        if gold is None or gold['dev'] is None or not 1 <= gold['longest'] <= _lib.SF_EVAL_MAX_GOLD:
            self.fallbacks += 1
            agent.test()
            return self.score_results(agent.results)
        import torch
        from .sweeps import epoch_minibatches
        env, dev = agent.env, self.table.dev.device
        env.reset_epoch()
        agent.losses, agent.results = [], {}
        walked = []                                           # (item, row, view, first action) per first occurrence
        for _, items, fresh in epoch_minibatches(env):
            rows, views = nav.start_states(items)
            first = agent._first_actions(nav, rows, views)
            walked += [(it, rows[b], views[b], 0 if first is None else first[b])
                       for b, it in enumerate(items) if fresh[b]]
        S, B, n = agent.walk_steps, len(walked), len(self.instr_ids)
        items, order, slots = [x[0] for x in walked], [], []
        for it in items:
            slots.append(len(order) if it['instr_id'] in self.instr_ids else -1)
            if slots[-1] >= 0:
                order.append(it['instr_id'])
        w = self._episode_words(nav, items, slots)
        i32 = w[[0, 1, 2, 4]].astype(np.int32)                # gold_id, scan_base, m, slot
        i64 = np.stack((np.arange(B), w[3]))                  # row_first, dist_off
        hop, base = nav.hop_rows(items) if agent.walk_policy == _lib.SF_WALK_SHORTEST else (None, None)
        with torch.cuda.device(dev):
            walk = nav.walk(agent.walk_policy, S, np.array([x[1] for x in walked], np.int32),
                            np.array([x[2] for x in walked], np.int32),
                            None if first is None else np.array([x[3] for x in walked], np.int32), hop, base)
            d32, d64 = torch.from_numpy(i32).to(dev), torch.from_numpy(i64).to(dev)
            out = _Outputs(dev, n, near_ld=gold['longest'] if self.coverage_metrics else 0)
            _, text = self._launch_route_scoring(out, 'walk', S=S, B=B, n_slots=n, row_stride=B, n_rows=(S + 1) * B,
                                                 row=walk['row'], row_first=d64[0], n_steps=walk['n_steps'],
                                                 actions=walk['actions'], gold_id=d32[0], scan_base=d32[1], m=d32[2],
                                                 dist_off=d64[1], slot=d32[3])
            out.download()
            down = [walk['err']] + ([walk['row'], walk['view'], walk['n_steps']] if keep_results else [])
            got = [torch.empty(x.shape, dtype=x.dtype).pin_memory() for x in down]
            for h, x in zip(got, down):
                h.copy_(x, non_blocking=True)
            torch.cuda.current_stream().synchronize()         # the one host sync of the sweep
        self.sweeps += 1
        self.last_host_syncs = 1
        self.host_syncs += 1
        if int(got[0][0]):
            raise agent.walk_error()
        out.check(text)
        self._assemble([self.gt[int(iid.split('_')[0])] for iid in order], *out.host(), lists=True)
        if keep_results:
            rows, views, steps = (x.numpy() for x in got[1:])
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
