// Path-fidelity scoring of navigation results on the device (speaker_follower_amd/evaluation.py, path_metrics): the six
// numbers of eval_score_kernel (sf_eval.hip) plus `shortest` = D[p_0][goal] and `dtw`, the dynamic-time-warping cost of
// the visited poses P = p_0 .. p_n against the gold path R = r_0 .. r_{g-1}:
//     C[0][0] = 0, C[a][0] = C[0][b] = inf otherwise, C[a][b] = D[p_{a-1}][r_{b-1}] + min(C[a-1][b], C[a][b-1], C[a-1][b-1])
// with the cost in the direction D[pred][gold], dtw = C[n+1][g].  Every cell is ONE rounded float64 add of one table
// element to an exact three-way minimum, so every evaluation order gives the same bits: the host runs the rows, this
// kernel the anti-diagonals.  Hence no contraction and no fast-math in this file, as in sf_eval.hip.
// With COVER (sf_eval_score_routes_coverage) the same launch also leaves near[b] = min over a of D[p_a][r_b] per gold
// node, the one route-dependent part of CLS: a minimum over the table elements the recurrence loads anyway, exact in
// any order.  The exponentials and the length score are formed on the host (evaluation.coverage_metrics_of).
#include "sf_common.h"

#pragma clang fp contract(off)

namespace sf {
namespace {

constexpr int ROUTES_PER_BLOCK = 4;    // one wavefront per route
constexpr int AHEAD = 8;               // anti-diagonals whose table elements are loaded before their cells are formed

// Lane l owns gold position l.  At anti-diagonal t it forms cell (a, l) with a = t - l the pose index: the left and the
// diagonal predecessor are lane l - 1's values of steps t - 1 and t - 2, the upper one is its own value of step t - 1.
// COVER: lane l < g also folds the costs of its cells into a minimum and stores it at near_out[slot * near_ld + l].
template <bool COVER>
__global__ __launch_bounds__(ROUTES_PER_BLOCK* WAVE) void eval_routes_kernel(sf_eval_routes p, int32_t* __restrict__ err,
                                                                            double* __restrict__ near_out, int32_t near_ld) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * ROUTES_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= p.B) return;                                    // (wave-uniform: no barrier in this kernel)
    const int slot = p.slot[b];
    if (slot == -1) return;
    const int m = p.m[b], base = p.scan_base[b], gid = p.gold_id[b];
    const int64_t first = p.row_first[b];
    const int64_t stride = p.row_stride;
    bool bad = slot < -1 || slot >= p.n_slots || m < 1 || (unsigned)gid >= (unsigned)p.n_gold || first < 0 ||
               first >= p.n_rows;
    int g = 0, g0 = 0;
    if (!bad) {
        g0 = p.gold_off[gid];
        g = p.gold_off[gid + 1] - g0;
        bad = g0 < 0 || g < 1 || g > SF_EVAL_MAX_GOLD || g0 > p.n_gold_nodes - g;
        if (COVER) bad = bad || g > near_ld;                 // (max_gold is a host copy: the row is checked here)
    }
    // the step count: given, or the first stop of actions [S, B] plus one, else S (sf_eval_score's rule)
    int n = 0;
    if (!bad) {
        if (p.n_steps) {
            n = p.n_steps[b];
        } else {
            n = p.S;
            for (int t0 = 0; t0 < p.S; t0 += WAVE) {
                const int t = t0 + lane;
                const bool stop = t < p.S && p.actions[(int64_t)t * p.B + b] == 0;
                const unsigned long long any = __ballot(stop);
                if (any) {
                    n = t0 + __ffsll(any);
                    break;
                }
            }
        }
        bad = n < 0 || n > 0x7fffffff - 2 * WAVE || n > (p.n_rows - 1 - first) / stride;
    }
    if (bad) {
        if (lane == 0) *err = 1;
        return;
    }
    // the gold path, one node per lane; every pose inside its scan, the first one the gold path's first node
    int gold = 0;
    if (lane < g) {
        gold = p.gold_node[g0 + lane];
        bad = (unsigned)gold >= (unsigned)m;
    }
    const double* D = p.table + p.dist_off[b];
    for (int t = lane; t <= n && !bad; t += WAVE) {
        const int r = p.row[first + (int64_t)t * stride] - base;
        bad = (unsigned)r >= (unsigned)m;
    }
    if (__any(bad)) {
        if (lane == 0) *err = 1;
        return;
    }
    const int start = p.row[first] - base;
    const int goal = __shfl(gold, g - 1, WAVE);
    if (start != __shfl(gold, 0, WAVE)) {
        if (lane == 0) *err = 1;
        return;
    }
    const double inf = __builtin_inf();
    // the classic six: the minimum over the path is exact in any order; the length is summed in path order, the edges
    // of 64 steps loaded at once and added one by one (every lane forms the same sum)
    double oracle = inf;
    for (int t = lane; t <= n; t += WAVE) {
        const int r = p.row[first + (int64_t)t * stride] - base;
        const double d = D[(int64_t)r * m + goal];
        if (d < oracle) oracle = d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(oracle, off, WAVE);
        if (o < oracle) oracle = o;
    }
    const int last = p.row[first + (int64_t)n * stride] - base;
    const double nav = D[(int64_t)last * m + goal];
    const double shortest = D[(int64_t)start * m + goal];
    double length = 0.0;
    for (int t0 = 0; t0 < n; t0 += WAVE) {
        const int t = t0 + lane;
        double edge = 0.0;
        if (t < n) {
            const int u = p.row[first + (int64_t)t * stride] - base;
            const int v = p.row[first + (int64_t)(t + 1) * stride] - base;
            edge = D[(int64_t)u * m + v];
        }
        const int cnt = n - t0 < WAVE ? n - t0 : WAVE;
        for (int i = 0; i < cnt; ++i) length = length + __shfl(edge, i, WAVE);
    }
    // the warping recurrence over n + g anti-diagonals; the table elements of the next AHEAD of them are in flight
    // while the cells of these AHEAD are formed (they depend on indices only)
    const int T = n + g;
    auto cost_of = [&](int t) -> double {
        const int a = t - lane;
        if (lane < g && a >= 0 && a <= n) {
            const int r = p.row[first + (int64_t)a * stride] - base;
            return D[(int64_t)r * m + gold];
        }
        return 0.0;
    };
    double cur = inf;                // C[a][l + 1] of the pose before: the upper predecessor; C[0][l + 1] = inf
    double diag = inf;               // lane l - 1's value of two steps ago
    double nearest = inf;            // COVER: the least cost of this lane's cells so far
    double cost[AHEAD], next[AHEAD];
#pragma unroll
    for (int i = 0; i < AHEAD; ++i) cost[i] = cost_of(i);
    for (int t0 = 0; t0 < T; t0 += AHEAD) {
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) next[i] = t0 + AHEAD < T ? cost_of(t0 + AHEAD + i) : 0.0;
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) {
            const int t = t0 + i;
            const int a = t - lane;
            double left = __shfl_up(cur, 1, WAVE);
            if (lane == 0) {                                 // column 0: C[0][0] = 0, C[a][0] = inf
                left = inf;
                diag = t == 0 ? 0.0 : inf;
            }
            if (lane < g && a >= 0 && a <= n) {
                double best = cur < left ? cur : left;
                best = diag < best ? diag : best;
                cur = cost[i] + best;
                if (COVER) nearest = cost[i] < nearest ? cost[i] : nearest;
            }
            diag = left;
        }
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) cost[i] = next[i];
    }
    const double dtw = __shfl(cur, g - 1, WAVE);
    if (lane == 0) {
        p.nav_error[slot] = nav;
        p.oracle_error[slot] = oracle;
        p.length[slot] = length;
        p.shortest[slot] = shortest;
        p.dtw[slot] = dtw;
        p.steps[slot] = n;
        p.success[slot] = nav < p.margin;
        p.oracle_success[slot] = oracle < p.margin;
    }
    if (COVER && lane < g) near_out[(int64_t)slot * near_ld + lane] = nearest;
}

}  // namespace
}  // namespace sf

static int score_routes(const sf_eval_routes* e, int32_t* err, double* near, int32_t near_ld, bool cover,
                        sf_stream stream) {
    SF_CHECK_ARG(e && err && e->B >= 1 && e->n_slots >= 1 && e->row_stride >= 1 && e->n_gold >= 1 && e->max_gold >= 1 &&
                 e->n_gold_nodes >= 1 && e->n_rows >= 1 && e->row && e->row_first && e->gold_off && e->gold_node &&
                 e->gold_id && e->scan_base && e->m && e->dist_off && e->slot && e->table && e->nav_error &&
                 e->oracle_error && e->length && e->shortest && e->dtw && e->steps && e->success && e->oracle_success);
    SF_CHECK_ARG(e->n_steps || (e->actions && e->S >= 1));
    SF_CHECK_ARG(!cover || (near && near_ld >= e->max_gold));
    if (e->max_gold > SF_EVAL_MAX_GOLD) return SF_ERR_UNSUPPORTED;
    const dim3 grid(sf::ceil_div(e->B, sf::ROUTES_PER_BLOCK)), block(sf::ROUTES_PER_BLOCK * sf::WAVE);
    if (cover) {
        SF_LAUNCH_AS("sf::eval_routes_kernel<cover>", sf::eval_routes_kernel<true>, grid, block, 0, (hipStream_t)stream, *e,
                     err, near, near_ld);
    } else {
        SF_LAUNCH_AS("sf::eval_routes_kernel", sf::eval_routes_kernel<false>, grid, block, 0, (hipStream_t)stream, *e, err,
                     (double*)nullptr, 0);
    }
    return sf::launch_status();
}

extern "C" int sf_eval_score_routes(const sf_eval_routes* e, int32_t* err, sf_stream stream) {
    SF_ENTER();
    return score_routes(e, err, nullptr, 0, false, stream);
}

extern "C" int sf_eval_score_routes_coverage(const sf_eval_routes* e, double* near, int32_t near_ld, int32_t* err,
                                             sf_stream stream) {
    SF_ENTER();
    return score_routes(e, err, near, near_ld, true, stream);
}
