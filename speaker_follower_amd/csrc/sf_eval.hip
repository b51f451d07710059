// Scoring of navigation results on the device (reference: tasks/R2R/eval.py:23-139): the all-pairs distance tables
// Evaluation.__init__ takes from networkx, and _score_item over the nav rows a device rollout recorded.
//
// Distances are the fixed point of the synchronous Bellman-Ford iteration in SOURCE-MAJOR orientation: D[s][v] =
// min(D[s][v], D[s][u] + w(u, v)).  With positive weights and monotone float64 rounding that system has exactly one
// solution, so the result is bit-equal to a Dijkstra search that accumulates d + w outward from s
// -- as long as every candidate is ONE rounded add.  Hence no contraction and no fast-math in this file.
#include "sf_common.h"

#pragma clang fp contract(off)

#include <atomic>

namespace sf {
namespace {

std::atomic<int> g_eval_max_nodes{SF_EVAL_MAX_NODES};

// One wavefront (= one workgroup) per source node.  Lane l owns the scan's nodes l, l + 64, ...; a round reads the
// previous round's vector and writes the other copy (Jacobi), the barrier between rounds is a one-wave barrier.
__global__ __launch_bounds__(WAVE) void eval_distances_kernel(sf_eval_graphs g, double* __restrict__ table,
                                                              int32_t* __restrict__ err) {
    __shared__ double dist[2][SF_EVAL_MAX_NODES];
    const int src_g = blockIdx.x;
    if (src_g >= g.n_nodes) return;
    // the scan that owns this source: the last k with node_off[k] <= src_g (uniform over the wave)
    int lo = 0, hi = g.n_scans - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g.node_off[mid] <= src_g) lo = mid; else hi = mid - 1;
    }
    const int base = g.node_off[lo];
    const int m = g.node_off[lo + 1] - base;
    if (m < 1 || m > SF_EVAL_MAX_NODES || src_g - base >= m) {      // (a table the launcher's checks cannot see)
        if (threadIdx.x == 0) *err = 1;
        return;
    }
    const int s = src_g - base;
    const int lane = threadIdx.x;
    const double inf = __builtin_inf();
    for (int v = lane; v < m; v += WAVE) dist[0][v] = v == s ? 0.0 : inf;
    __syncthreads();
    int cur = 0, changed = 0;
    for (int round = 0; round < m; ++round) {
        const double* d = dist[cur];
        double* nd = dist[cur ^ 1];
        int mine = 0;
        for (int v = lane; v < m; v += WAVE) {
            const double old = d[v];
            double best = old;
            const int e1 = g.edge_off[base + v + 1];
            for (int e = g.edge_off[base + v]; e < e1; ++e) {
                const int u = g.edge_src[e];
                if ((unsigned)u >= (unsigned)m) { mine = 2; continue; }
                const double c = d[u] + g.edge_w[e];
                if (c < best) best = c;
            }
            nd[v] = best;
            mine |= best != old;
        }
        changed = __syncthreads_or(mine);
        cur ^= 1;
        if (!(changed & 1)) break;
    }
    if (changed && lane == 0) *err = 1;          // round m still moved a value, or an edge left its scan
    double* out = table + g.dist_off[lo] + (int64_t)s * m;
    for (int v = lane; v < m; v += WAVE) out[v] = dist[cur][v];
}

// One thread per episode.
__global__ __launch_bounds__(256) void eval_score_kernel(sf_eval_episodes p, int32_t* __restrict__ err) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const int slot = p.slot[b];
    if (slot == -1) return;
    const int m = p.m[b], base = p.scan_base[b];
    const int goal = p.goal_row[b] - base;
    if (slot < -1 || slot >= p.n_slots || m < 1 || (unsigned)goal >= (unsigned)m) {
        *err = 1;
        return;
    }
    int n = p.S;
    for (int t = 0; t < p.S; ++t)
        if (p.actions[(int64_t)t * p.B + b] == 0) { n = t + 1; break; }
    const double* D = p.table + p.dist_off[b];
    double nav = 0.0, oracle = 0.0, length = 0.0;
    int prev = 0;
    for (int t = 0; t <= n; ++t) {
        const int r = p.row[(int64_t)t * p.B + b] - base;
        if ((unsigned)r >= (unsigned)m) {
            *err = 1;
            return;
        }
        const double d = D[(int64_t)r * m + goal];
        if (t == 0 || d < oracle) oracle = d;
        if (t > 0) length = length + D[(int64_t)prev * m + r];
        nav = d;
        prev = r;
    }
    p.nav_error[slot] = nav;
    p.oracle_error[slot] = oracle;
    p.length[slot] = length;
    p.steps[slot] = n;
    p.success[slot] = nav < p.margin;
    p.oracle_success[slot] = oracle < p.margin;
}

}  // namespace
}  // namespace sf

extern "C" size_t sf_eval_distances_bytes(const int32_t* m, int n_scans) {
    if (!m || n_scans < 1) return 0;
    size_t total = 0;
    for (int k = 0; k < n_scans; ++k) {
        if (m[k] < 0) return 0;
        total += (size_t)m[k] * (size_t)m[k] * sizeof(double);
    }
    return total;
}

extern "C" int sf_eval_max_nodes(void) { return sf::g_eval_max_nodes.load(); }

extern "C" void sf_debug_eval_max_nodes(int n) {
    sf::g_eval_max_nodes.store(n >= 1 && n <= SF_EVAL_MAX_NODES ? n : SF_EVAL_MAX_NODES);
}

extern "C" int sf_eval_distances(const sf_eval_graphs* g, double* table, int32_t* err, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(g && table && err && g->node_off && g->edge_off && g->edge_src && g->edge_w && g->dist_off &&
                 g->n_scans >= 1 && g->n_nodes >= 1 && g->max_nodes >= 1 && g->max_nodes <= g->n_nodes);
    if (g->max_nodes > sf_eval_max_nodes()) return SF_ERR_UNSUPPORTED;
    SF_LAUNCH(sf::eval_distances_kernel, dim3(g->n_nodes), dim3(sf::WAVE), 0, (hipStream_t)stream, *g, table, err);
    return sf::launch_status();
}

extern "C" int sf_eval_score(const sf_eval_episodes* e, int32_t* err, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(e && err && e->S >= 1 && e->B >= 1 && e->n_slots >= 1 && e->row && e->actions && e->goal_row &&
                 e->scan_base && e->m && e->dist_off && e->slot && e->table && e->nav_error && e->oracle_error &&
                 e->length && e->steps && e->success && e->oracle_success);
    SF_LAUNCH(sf::eval_score_kernel, dim3(sf::ceil_div(e->B, 256)), dim3(256), 0, (hipStream_t)stream, *e, err);
    return sf::launch_status();
}
