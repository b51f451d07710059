// Device-resident navigation: env.step + env.observe + the shortest-path teacher of a whole batch as
// ONE small launch per decode step (reference: R2RBatch.step / observe / _shortest_path_action,
// tasks/R2R/env.py:628-641, 742-761, 763-804; the panorama sweep behind the candidate lists,
// env.py:149-224, is a pure function of (viewpoint, view index) and is tabulated once on the host).
// With it a student-forced rollout on REAL connectivity graphs needs no host round trip per step:
// the glue kernel leaves a_t on the device, this kernel turns (state, a_t) into the next state and
// writes the next step's index-form observation where the decoder kernels read it.
#include "sf_kernels.h"
#include "sf_glue.h"

namespace sf {
namespace {

// one thread per (sample, candidate slot)
__global__ __launch_bounds__(256) void nav_step_kernel(NavIO p, int B, const int64_t* a_t, const uint8_t* ended) {
    const int A = p.nav.A;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * A) return;
    const int b = i / A, a = i - b * A;
    int act = -1;
    if (a_t) {
        act = (int)a_t[b];
        act = act < 0 ? 0 : act;
    }
    nav_advance_slot(p, b, a, act, ended && ended[b]);
}

constexpr int WALKS_PER_BLOCK = 4;     // one wavefront per episode

// A whole episode of a table-driven policy (sf_nav_walk): the state transition is nav_advance_slot's, the teacher its
// target rule.  Lane c owns candidate slot c of the current state: one step is one round of look-ups (a_num, the state's
// next_row / cand_view rows and the hop, all addressed by the state alone) and a ballot.  Lane 0 stores; after the
// stop the lanes fill what is left of the row's columns, so every element is written.
__global__ __launch_bounds__(WALKS_PER_BLOCK* WAVE) void nav_walk_kernel(
    sf_nav_table nav, int policy, int B, int S, const int32_t* __restrict__ row0, const int32_t* __restrict__ view0,
    const int32_t* __restrict__ first_action, const int32_t* __restrict__ goal_hop, int ld_hop,
    const int32_t* __restrict__ hop_base, int32_t* __restrict__ row_out, int32_t* __restrict__ view_out,
    int64_t* __restrict__ actions, int32_t* __restrict__ n_steps, int32_t* __restrict__ err) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * WALKS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= B) return;                                      // (wave-uniform: no barrier in this kernel)
    const int A = nav.A, V = nav.V;
    const int start_row = row0[b], start_view = view0[b];
    int row = start_row, view = start_view;
    bool bad = (unsigned)view >= (unsigned)V;
    const int base = policy == SF_WALK_SHORTEST ? hop_base[b] : 0;
    const int first = policy == SF_WALK_RANDOM ? first_action[b] : 0;
    if (lane == 0) {
        row_out[b] = row;
        view_out[b] = view;
    }
    int k = 0;                                               // actions taken so far; the one at k - 1 ended the walk
    bool stopped = bad;
    while (!stopped && k < S) {
        const size_t s = (size_t)row * V + view;
        int n = nav.a_num[s];
        n = n > A ? A : n;
        int nr = -1, cv = 0;
        if (lane < A) {
            nr = nav.next_row[s * A + lane];
            cv = nav.cand_view[s * A + lane];
        }
        int act = 0;
        if (policy == SF_WALK_SHORTEST) {
            const int hop = goal_hop[(size_t)b * ld_hop + (row - base)];
            if (hop != row) {                                // the first candidate that leads to the hop, else stop
                const unsigned long long leads = __ballot(lane >= 1 && lane < n && nr == hop);
                act = leads ? __ffsll(leads) - 1 : 0;
            }
        } else if (policy == SF_WALK_RANDOM) {
            if (k == 0) {
                act = first;
                bad = act < 1 || act >= n;
            } else if (k < SF_WALK_RANDOM_MOVES) {
                act = 1;
                bad = n <= 1;
            }
            if (bad) break;
        }
        if (act != 0) {
            const int to = __shfl(nr, act, WAVE);
            if (to != row) {                                 // (a candidate that is the current viewpoint stays)
                view = __shfl(cv, act, WAVE);
                row = to;
            }
        }
        if (lane == 0) {
            actions[(int64_t)k * B + b] = act;
            row_out[(int64_t)(k + 1) * B + b] = row;
            view_out[(int64_t)(k + 1) * B + b] = view;
        }
        ++k;
        stopped = act == 0;
    }
    int n_out;
    if (bad) {                                               // nothing of the row's walk stands: the start state throughout
        row = start_row;
        view = start_view;
        if (lane == 0) {                                     // (the lane that wrote them rewrites them: k <= 4)
            *err = 1;
            for (int t = 0; t < k; ++t) {
                actions[(int64_t)t * B + b] = 0;
                row_out[(int64_t)(t + 1) * B + b] = row;
                view_out[(int64_t)(t + 1) * B + b] = view;
            }
        }
        n_out = -1;
    } else if (policy == SF_WALK_SHORTEST) {                 // the last observation is dropped, cut off or not
        const int stop_at = stopped ? k - 1 : S;
        n_out = stop_at < S - 1 ? stop_at : S - 1;
    } else {
        n_out = k - 1;                                       // STOP: 0; RANDOM: its moves
    }
    for (int t = k + lane; t < S; t += WAVE) {
        actions[(int64_t)t * B + b] = 0;
        row_out[(int64_t)(t + 1) * B + b] = row;
        view_out[(int64_t)(t + 1) * B + b] = view;
    }
    if (lane == 0) n_steps[b] = n_out;
}

// ---- sf_nav_routes: the shortest-path routes of a split, as lengths or as the speaker's packed minibatches ----------

__host__ __device__ inline int64_t align8(int64_t x) { return (x + 7) & ~(int64_t)7; }

// speaker.packed_layout(B, Tp, Lmax): the byte offset of every section of a block, and the block's size
struct RouteLayout {
    int64_t vp, view, act, act_view, sincos, mask, bytes;    // (instr_seq stands at 0)
};
__host__ __device__ inline RouteLayout route_layout(int B, int Tp, int Lmax) {
    RouteLayout l;
    const int64_t grid = (int64_t)Tp * B * 4;
    l.vp = align8((int64_t)B * Lmax * 8);
    l.view = align8(l.vp + grid);
    l.act = align8(l.view + grid);
    l.act_view = align8(l.act + grid);
    l.sincos = align8(l.act_view + grid);
    l.mask = align8(l.sincos + grid * 4);
    l.bytes = align8(l.mask + (int64_t)B * Tp);
    return l;
}

// column `col` of a block's sections (pack mode), or all NULL
struct RouteCols {
    int64_t* seq;
    int32_t *vp, *view, *act, *act_view;
    uint32_t* sincos;                                        // (bit patterns: the table's floats are copied, not computed)
    uint8_t* mask;
    int B, Tp, col;
};

// lanes 0 .. 3: step t of the column; `from` = the table's four values of a move, NULL for a stop or a dead step
__device__ __forceinline__ void route_store_step(const RouteCols& c, int lane, int t, int vp, int view, int act_view,
                                                 const uint32_t* from) {
    const int64_t at = (int64_t)t * c.B + c.col;
    if (lane == 0) {
        c.vp[at] = vp;
        c.view[at] = view;
        c.act[at] = from != nullptr;
        c.act_view[at] = act_view;
    }
    if (lane < 4) c.sincos[at * 4 + lane] = from ? from[lane] : ((lane & 1) ? 0x3f800000u : 0u);   // (0, 1, 0, 1)
}

// One walk of route r's teacher from (row, view).  WRITE = false: nothing is stored, the walk is only measured (k
// actions, `stopped` by an action 0, `bad` on a row outside the route's hop block).  WRITE = true (a walk already
// measured: not bad, and in pack mode k <= Tp): rows and the column's live steps are stored as it goes.
template <bool WRITE>
__device__ __forceinline__ void route_walk(const sf_nav_table& nav, const sf_nav_routes_io& p, const RouteCols& c, int slot,
                                           int lane, int base, int m, const int32_t* __restrict__ hop_row, int& row,
                                           int& view, int& k, bool& stopped, bool& bad) {
    const int A = nav.A, V = nav.V;
    k = 0;
    stopped = false;
    while (!stopped && k < p.S) {
        const unsigned local = (unsigned)(row - base);
        if (local >= (unsigned)m) {
            bad = true;
            return;
        }
        const size_t s = (size_t)row * V + view;
        int n = nav.a_num[s];
        n = n > A ? A : n;
        int nr = -1, cv = 0;
        if (lane < A) {
            nr = nav.next_row[s * A + lane];
            cv = nav.cand_view[s * A + lane];
        }
        const int hop = hop_row[local];
        int act = 0;
        if (hop != row) {                                    // the first candidate that leads to the hop, else stop
            const unsigned long long leads = __ballot(lane >= 1 && lane < n && nr == hop);
            act = leads ? __ffsll(leads) - 1 : 0;
        }
        const int to = __shfl(nr, act, WAVE), to_view = __shfl(cv, act, WAVE);
        if (WRITE && c.vp)
            route_store_step(c, lane, k, nav.feat_row[row], view, act ? to_view : 0,
                             act ? (const uint32_t*)nav.cand_sincos + (s * A + act) * 4 : nullptr);
        if (act != 0 && to != row) {                         // (a candidate that is the current viewpoint stays)
            view = to_view;
            row = to;
        }
        ++k;
        if (WRITE && p.rows && lane == 0) p.rows[(int64_t)k * p.n_slots + slot] = row;
        stopped = act == 0;
    }
}

__global__ __launch_bounds__(WALKS_PER_BLOCK* WAVE) void nav_routes_kernel(sf_nav_table nav, sf_nav_routes_io p,
                                                                           int32_t* __restrict__ err) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int slot = blockIdx.x * WALKS_PER_BLOCK + (threadIdx.x >> 6);
    if (slot >= p.n_slots) return;                           // (wave-uniform: no barrier in this kernel)
    const int S = p.S;
    RouteCols c = {};
    if (p.out) {
        const int i = slot / p.B;
        c.B = p.B;
        c.col = slot - i * p.B;
        c.Tp = p.mb_Tp_dev[i];
        const int64_t off = p.mb_off_dev[i];
        if (c.Tp < 1 || c.Tp > S || off < 0 || (off & 7) || off > p.out_bytes ||
            route_layout(p.B, c.Tp, p.Lmax).bytes > p.out_bytes - off) {
            if (lane == 0) *err = 1;                         // not what the entry checked: the minibatch is left alone
            return;
        }
        const RouteLayout l = route_layout(p.B, c.Tp, p.Lmax);
        uint8_t* blk = p.out + off;
        c.seq = (int64_t*)blk + (int64_t)c.col * p.Lmax;
        c.vp = (int32_t*)(blk + l.vp);
        c.view = (int32_t*)(blk + l.view);
        c.act = (int32_t*)(blk + l.act);
        c.act_view = (int32_t*)(blk + l.act_view);
        c.sincos = (uint32_t*)(blk + l.sincos);
        c.mask = blk + l.mask + (int64_t)c.col * c.Tp;
    }
    const int r = p.route ? p.route[slot] : slot;
    const bool known = (unsigned)r < (unsigned)p.N;
    int start_row = 0, start_view = 0, base = 0, m = 0, goal = -1;
    const int32_t* hop_row = p.hop_all;
    if (known) {
        start_row = p.row0[r];
        start_view = p.view0[r];
        base = p.hop_base[r];
        m = p.hop_rows[r];
        goal = p.goal[r];
        hop_row += p.hop_off[r];
    }
    const bool row_ok = known && (unsigned)(start_row - base) < (unsigned)m;
    bool bad = !row_ok || (unsigned)start_view >= (unsigned)nav.V, stopped = false;
    int row = start_row, view = start_view, k = 0;
    if (!bad) route_walk<false>(nav, p, c, slot, lane, base, m, hop_row, row, view, k, stopped, bad);
    const int n_out = bad ? 1 : k;
    const int did_reach = !bad && stopped && row == goal;
    const bool refused = bad || (c.vp && k > c.Tp);          // the column (and, if bad, the rows) hold one stop at the start
    if (refused && lane == 0) *err = 1;
    if (lane == 0 && p.rows) p.rows[slot] = start_row;
    int n_live = 1;                                          // live steps of the column
    if (!refused || !bad) {                                  // the walk again, this time stored
        RouteCols cw = c;
        if (refused) cw.vp = nullptr;                        // (too long for its block: its rows only)
        row = start_row;
        view = start_view;
        route_walk<true>(nav, p, cw, slot, lane, base, m, hop_row, row, view, k, stopped, bad);
        if (!refused) n_live = k;
    } else {
        row = start_row;
        k = 0;
    }
    if (p.rows)
        for (int t = k + 1 + lane; t <= S; t += WAVE) p.rows[(int64_t)t * p.n_slots + slot] = row;
    if (lane == 0 && p.n_actions) {
        p.n_actions[slot] = n_out;
        p.reached[slot] = did_reach;
    }
    if (!c.vp) return;
    if (refused) route_store_step(c, lane, 0, row_ok ? nav.feat_row[start_row] : -1, start_view, 0, nullptr);
    for (int t = n_live + lane; t < c.Tp; t += WAVE) {       // dead steps: a lane per step
        const int64_t at = (int64_t)t * c.B + c.col;
        c.vp[at] = -1;
        c.view[at] = 0;
        c.act[at] = 0;
        c.act_view[at] = 0;
        for (int q = 0; q < 4; ++q) c.sincos[at * 4 + q] = (q & 1) ? 0x3f800000u : 0u;
    }
    for (int t = lane; t < c.Tp; t += WAVE) c.mask[t] = t >= n_live;
    int64_t first = 0, len = 0;
    if (p.instr_tokens && known) {
        first = p.instr_off[r];
        len = p.instr_off[r + 1] - first;
        len = len < 0 ? 0 : len;
    }
    const int L = p.Lmax;
    const int64_t kept = len < L - 1 ? len : L - 1;          // follower.py:75-105, reverse = False
    for (int j = lane; j < L; j += WAVE) {
        int64_t w = p.pad;
        if (j < kept) w = p.instr_tokens[first + j];
        else if (len + 1 <= L ? j == kept : j == L - 1) w = len + 1 <= L ? (int64_t)p.eos : p.instr_tokens[first + L - 1];
        c.seq[j] = w;
    }
}

// ---- sf_nav_follower_batches: the follower's minibatches of a route set, sorted and padded as the host path does -----

constexpr int FOLLOWER_MAX_B = 1024;   // raw lengths and column slots in LDS: 2 x 4 KB
constexpr int FOLLOWER_THREADS = 256;

__host__ __device__ inline int64_t align64(int64_t x) { return (x + 63) & ~(int64_t)63; }

// nav.DeviceNavBatch.pack_layout(B, Lmax, ld): the byte offset of every section of a block, and the block's size
struct FollowerLayout {
    int64_t mask, lengths, rows, views, hop, base, bytes;    // (seq stands at 0)
};
__host__ __device__ inline FollowerLayout follower_layout(int B, int Lmax, int ld) {
    FollowerLayout l;
    l.mask = align64((int64_t)B * Lmax * 8);
    l.lengths = align64(l.mask + (int64_t)B * Lmax);
    l.rows = align64(l.lengths + (int64_t)B * 4);
    l.views = align64(l.rows + (int64_t)B * 4);
    l.hop = align64(l.views + (int64_t)B * 4);
    l.base = align64(l.hop + (int64_t)B * ld * 4);
    l.bytes = align64(l.base + (int64_t)B * 4);
    return l;
}

// what slot j of the launch holds: its route, whether the index is one, its token count and whether the column is
// written as an empty instruction
struct FollowerSlot {
    int r, raw;
    int64_t first;
    bool known, bad;
};
__device__ __forceinline__ FollowerSlot follower_slot(const sf_nav_follower_io& p, int64_t j) {
    FollowerSlot s;
    s.r = p.order[j];
    s.known = (unsigned)s.r < (unsigned)p.N;
    s.raw = 0;
    s.first = 0;
    s.bad = !s.known;
    if (s.known) {
        s.bad = (unsigned)p.view0[s.r] >= (unsigned)p.V || p.hop_rows[s.r] > p.ld;
        if (p.instr_tokens) {
            s.first = p.instr_off[s.r];
            int64_t len = p.instr_off[s.r + 1] - s.first;
            len = len < 0 ? 0 : (len > 0x7ffffffe ? 0x7ffffffe : len);
            s.raw = (int)len;
            if (len > 0 && p.instr_tokens[s.first + len - 1] == (int64_t)p.eos) s.bad = true;
        }
    }
    if (s.bad) s.raw = 0;
    return s;
}

__global__ __launch_bounds__(FOLLOWER_THREADS) void nav_follower_batches_kernel(sf_nav_follower_io p,
                                                                                int32_t* __restrict__ err) {
    __shared__ int raw[FOLLOWER_MAX_B];
    __shared__ int slot_of[FOLLOWER_MAX_B];                  // column -> slot of the minibatch
    const int i = blockIdx.x, B = p.B, L = p.Lmax, ld = p.ld;
    const int64_t off = p.mb_off_dev[i];
    const FollowerLayout l = follower_layout(B, L, ld);
    if (off < 0 || (off & 63) || off > p.out_bytes || l.bytes > p.out_bytes - off) {   // (block-uniform)
        if (threadIdx.x == 0) *err = 1;                      // not what the entry checked: the minibatch is left alone
        return;
    }
    const int64_t slot0 = (int64_t)i * B;
    for (int j = threadIdx.x; j < B; j += FOLLOWER_THREADS) {
        const FollowerSlot s = follower_slot(p, slot0 + j);
        if (s.bad) *err = 1;
        raw[j] = s.raw;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < B; j += FOLLOWER_THREADS) {
        const int mine = raw[j];
        int col = 0;
        for (int q = 0; q < B; ++q) col += raw[q] > mine || (raw[q] == mine && q < j);
        slot_of[col] = j;                                    // (the columns are a permutation of the slots)
    }
    __syncthreads();
    uint8_t* blk = p.out + off;
    int64_t* seq = (int64_t*)blk;
    uint8_t* mask = blk + l.mask;
    int32_t* lengths = (int32_t*)(blk + l.lengths);
    int32_t* rows = (int32_t*)(blk + l.rows);
    int32_t* views = (int32_t*)(blk + l.views);
    int32_t* hop = (int32_t*)(blk + l.hop);
    int32_t* base = (int32_t*)(blk + l.base);
    const int lane = threadIdx.x & (WAVE - 1);
    for (int c = threadIdx.x >> 6; c < B; c += FOLLOWER_THREADS / WAVE) {   // a wavefront per column
        const FollowerSlot s = follower_slot(p, slot0 + slot_of[c]);
        const int len = s.raw;
        const int kept = len + 1 < L ? len + 1 : L;
        for (int k = lane; k < L; k += WAVE) {
            int64_t w = p.pad;
            if (k < len) w = p.instr_tokens[s.first + (p.reverse ? len - 1 - k : k)];
            else if (k == len) w = p.eos;
            seq[(int64_t)c * L + k] = w;
            mask[(int64_t)c * L + k] = w == (int64_t)p.pad;
        }
        int m = 0;
        const int32_t* from = p.hop_all;
        if (s.known) {
            m = p.hop_rows[s.r];
            m = m > ld ? ld : m;
            from += p.hop_off[s.r];
        }
        for (int k = lane; k < ld; k += WAVE) hop[(int64_t)c * ld + k] = k < m ? from[k] : 0;
        if (lane == 0) {
            lengths[c] = kept;
            rows[c] = s.known ? p.row0[s.r] : 0;
            views[c] = s.known ? p.view0[s.r] : 0;
            base[c] = s.known ? p.hop_base[s.r] : 0;
            if (p.col_route) {
                p.col_route[slot0 + c] = s.r;
                p.col_len[slot0 + c] = kept;
            }
        }
    }
}

}  // namespace

int nav_follower_batches(const sf_nav_follower_io* io, int32_t* err, hipStream_t st) {
    SF_LAUNCH(nav_follower_batches_kernel, dim3(io->M), dim3(FOLLOWER_THREADS), 0, st, *io, err);
    return launch_status();
}

int nav_routes(const sf_nav_table* nav, const sf_nav_routes_io* io, int32_t* err, hipStream_t st) {
    SF_LAUNCH(nav_routes_kernel, dim3(ceil_div(io->n_slots, WALKS_PER_BLOCK)), dim3(WALKS_PER_BLOCK * WAVE), 0, st, *nav, *io,
              err);
    return launch_status();
}

int nav_step(const sf_nav_table* nav, int B, const int32_t* row, const int32_t* view, const int64_t* a_t,
             const uint8_t* ended, const int32_t* goal_hop, int ld_hop, const int32_t* hop_base,
             int32_t* row_next, int32_t* vp_next, int32_t* view_next, int32_t* a_num_next,
             int32_t* cand_view_next, float* sincos_next, int64_t* target_next, hipStream_t st) {
    NavIO p{*nav, row, view, goal_hop, ld_hop, hop_base, row_next, vp_next, view_next, a_num_next, cand_view_next,
            sincos_next, target_next, true};
    SF_LAUNCH(nav_step_kernel, dim3(ceil_div(B * nav->A, 256)), dim3(256), 0, st, p, B, a_t, ended);
    return launch_status();
}

int nav_walk(const sf_nav_table* nav, int policy, int B, int S, const int32_t* row0, const int32_t* view0,
             const int32_t* first_action, const int32_t* goal_hop, int ld_hop, const int32_t* hop_base, int32_t* row,
             int32_t* view, int64_t* actions, int32_t* n_steps, int32_t* err, hipStream_t st) {
    SF_LAUNCH(nav_walk_kernel, dim3(ceil_div(B, WALKS_PER_BLOCK)), dim3(WALKS_PER_BLOCK * WAVE), 0, st, *nav, policy, B, S,
              row0, view0, first_action, goal_hop, ld_hop, hop_base, row, view, actions, n_steps, err);
    return launch_status();
}

}  // namespace sf

extern "C" int sf_nav_walk(const sf_nav_table* nav, int policy, int B, int S, const int32_t* row0, const int32_t* view0,
                           const int32_t* first_action, const int32_t* goal_hop, int ld_hop, const int32_t* hop_base,
                           int32_t* row, int32_t* view, int64_t* actions, int32_t* n_steps, int32_t* err,
                           sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(nav && nav->a_num && nav->next_row && nav->cand_view && nav->A > 0 && nav->V > 0 && B >= 1 && S >= 1 &&
                 row0 && view0 && row && view && actions && n_steps && err);
    SF_CHECK_ARG(policy == SF_WALK_STOP || policy == SF_WALK_SHORTEST || policy == SF_WALK_RANDOM);
    SF_CHECK_ARG(policy != SF_WALK_SHORTEST || (goal_hop && hop_base && ld_hop > 0));
    SF_CHECK_ARG(policy != SF_WALK_RANDOM || (first_action && S >= SF_WALK_RANDOM_MOVES + 1));
    if (nav->A > 64) return SF_ERR_UNSUPPORTED;              // one lane per candidate slot
    return sf::nav_walk(nav, policy, B, S, row0, view0, first_action, goal_hop, ld_hop, hop_base, row, view, actions,
                        n_steps, err, (hipStream_t)stream);
}

extern "C" int sf_nav_routes(const sf_nav_table* nav, const sf_nav_routes_io* io, int32_t* err, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(nav && io && err && nav->a_num && nav->next_row && nav->cand_view && nav->A > 0 && nav->V > 0);
    SF_CHECK_ARG(io->N >= 1 && io->S >= 1 && io->n_slots >= 1 && io->row0 && io->view0 && io->goal && io->hop_all &&
                 io->hop_off && io->hop_base && io->hop_rows);
    if (!io->out) {
        SF_CHECK_ARG(io->n_actions && io->reached && io->rows);
    } else {
        SF_CHECK_ARG(nav->cand_sincos && nav->feat_row && io->B >= 1 && io->Lmax >= 1 && io->M >= 1 &&
                     (int64_t)io->M * io->B == io->n_slots && io->out_bytes >= 1 && io->mb_Tp && io->mb_off &&
                     io->mb_Tp_dev && io->mb_off_dev);
        SF_CHECK_ARG(!io->n_actions == !io->reached && !io->n_actions == !io->rows);
        SF_CHECK_ARG(!io->instr_tokens == !io->instr_off);
        for (int i = 0; i < io->M; ++i) {
            const int Tp = io->mb_Tp[i];
            const int64_t off = io->mb_off[i];
            SF_CHECK_ARG(Tp >= 1 && Tp <= io->S && off >= 0 && !(off & 7) && off <= io->out_bytes &&
                         sf::route_layout(io->B, Tp, io->Lmax).bytes <= io->out_bytes - off);
        }
    }
    if (nav->A > 64) return SF_ERR_UNSUPPORTED;              // one lane per candidate slot
    return sf::nav_routes(nav, io, err, (hipStream_t)stream);
}

extern "C" int sf_nav_follower_batches_max_b(void) { return sf::FOLLOWER_MAX_B; }

extern "C" int sf_nav_follower_batches(const sf_nav_follower_io* io, int32_t* err, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(io && err && io->row0 && io->view0 && io->hop_all && io->hop_off && io->hop_base && io->hop_rows &&
                 io->order && io->mb_off && io->mb_off_dev && io->out);
    SF_CHECK_ARG(io->N >= 1 && io->V >= 1 && io->B >= 1 && io->Lmax >= 1 && io->ld >= 1 && io->M >= 1);
    SF_CHECK_ARG(!io->instr_tokens == !io->instr_off && !io->col_route == !io->col_len);
    SF_CHECK_ARG(((uintptr_t)io->out & 7) == 0);                  // (seq is stored as int64 words)
    const int64_t bytes = sf::follower_layout(io->B, io->Lmax, io->ld).bytes;
    for (int i = 0; i < io->M; ++i) {
        const int64_t off = io->mb_off[i];
        SF_CHECK_ARG(off >= 0 && !(off & 63) && off <= io->out_bytes && bytes <= io->out_bytes - off);
    }
    if (io->B > sf::FOLLOWER_MAX_B) return SF_ERR_UNSUPPORTED;    // raw lengths and column slots live in LDS
    return sf::nav_follower_batches(io, err, (hipStream_t)stream);
}

extern "C" int sf_nav_step(const sf_nav_table* nav, int B, const int32_t* row, const int32_t* view,
                           const int64_t* a_t, const uint8_t* ended, const int32_t* goal_hop, int ld_hop,
                           const int32_t* hop_base, int32_t* row_next, int32_t* vp_next, int32_t* view_next,
                           int32_t* a_num_next, int32_t* cand_view_next, float* sincos_next,
                           int64_t* target_next, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(nav && nav->a_num && nav->next_row && nav->cand_view && nav->cand_sincos && nav->feat_row &&
                 nav->A > 0 && nav->V > 0 && B > 0 && row && view && row_next && vp_next && view_next &&
                 a_num_next && cand_view_next && sincos_next && (!target_next || (goal_hop && hop_base && ld_hop > 0)));
    return sf::nav_step(nav, B, row, view, a_t, ended, goal_hop, ld_hop, hop_base, row_next, vp_next, view_next,
                        a_num_next, cand_view_next, sincos_next, target_next, (hipStream_t)stream);
}
