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

}  // namespace

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
