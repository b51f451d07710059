// The beam selections on the device: one decode step's choice of the next hypotheses of every instance, so that the
// step loop of a beam search runs without a host round trip per step.
//   * the speaker's (reference: Seq2SeqSpeaker.beam_search, tasks/R2R/speaker.py:262-296; search.DeviceSpeakerBeam),
//     layout contract: include/sf_hip.h, sf_speaker_beam_select;
//   * the follower's (reference: Seq2SeqAgent.beam_search, tasks/R2R/follower.py:606-690; search.DeviceFollowerBeam),
//     layout contract: include/sf_hip.h, sf_follower_beam_select.
//
// One wavefront per instance.  Lane i holds the i-th live slot of the instance; its k successors arrive from
// sf_logprob_topk already in descending order (ties: lower column first), so slot i's candidates
// score[i] + lp[i, j] are sorted by (score desc, flat index i*k+j asc) and the beam_size best of the instance are
// a merge of at most 64 sorted lists: beam_size rounds of a wave-wide arg-max over the list heads.
//
// Both kernels are the same four stages -- beam_merge, beam_place, beam_copy_attention, beam_close -- around what is
// their own: what ends a successor list, what a selection carries (a word; an action and the state it leads to) and
// which slot arrays the next step reads.  A stage takes the kernel's struct as a template parameter where it touches
// the fields sf_spk_beam and sf_fol_beam share by name.
#include "sf_kernels.h"

namespace sf {
namespace {

constexpr int BEAM_WAVE = 64;           // one lane per slot: beam_size <= 64

// (score, flat) of `o` comes before (score, flat) of the current best: higher score, then lower flat index.
// An empty head is (-inf, INT_MAX): every real candidate, a -inf one included, comes before it.
__device__ __forceinline__ bool beam_before(float os, int of, float bs, int bf) {
    return os > bs || (os == bs && of < bf);
}

// The merge of the live slots' sorted successor lists.  my_score / my_lp: this lane's hypothesis score and its k
// log-probabilities; valid(j): rank j is a successor (a list ends at the first rank that is none).  Leaves (slot inside
// the instance, rank, score) of selection q in s_row / s_rank / s_score [q] and returns the number of selections, after
// a barrier: every global read the caller made before the call happened before any write it makes after it.
template <class Valid>
__device__ __forceinline__ int beam_merge(int lane, int live, int W, int k, float my_score, const float* my_lp,
                                          Valid valid, int* s_row, int* s_rank, float* s_score) {
    int j = 0;
    float head;                                           // the head's score (one float32 add, as the reference's)
    int head_flat;
    auto load_head = [&] {
        head = -INFINITY;
        head_flat = 0x7fffffff;
        if (lane < live && j < k && valid(j)) {
            head = my_score + my_lp[j];
            head_flat = lane * k + j;
        }
    };
    load_head();
    int nsel = 0;
    for (; nsel < W; ++nsel) {
        float bs = fmaxf(head, -INFINITY);                // (ordering key: a NaN sorts last, the order stays total)
        int bf = head_flat;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(bs, off, BEAM_WAVE);
            const int of = __shfl_xor(bf, off, BEAM_WAVE);
            if (beam_before(os, of, bs, bf)) {
                bs = os;
                bf = of;
            }
        }
        if (bf == 0x7fffffff) break;                      // every list is exhausted (fewer successors than beam_size)
        if (bf == head_flat) {                            // this lane's head won: record it, advance the list
            s_row[nsel] = lane;
            s_rank[nsel] = j;
            s_score[nsel] = head;
            ++j;
            load_head();
        }
    }
    __syncthreads();
    return nsel;
}

// Where selection `lane` goes: the continuing hypotheses first, then the finals, both in selection order.
struct BeamPlace {
    int h;                                                // its history position (and, continuing, its next slot)
    int done_after, live_next;                            // the instance's completions and live slots after the step
};

// `fin` implies `sel`.  Appends the finals to the instance's completion list (done_rec / done_score).
template <class S>
__device__ __forceinline__ BeamPlace beam_place(const S& s, int b, int lane, int t, int n_done, bool sel, bool fin,
                                                float score) {
    const int W = s.beam_size;
    const unsigned long long m_fin = __ballot(fin), m_cont = __ballot(sel && !fin);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_fin = __popcll(m_fin), n_cont = __popcll(m_cont);
    BeamPlace p;
    p.h = b * W + (fin ? n_cont + __popcll(m_fin & below) : __popcll(m_cont & below));
    p.done_after = n_done + n_fin;
    p.live_next = p.done_after >= W ? 0 : n_cont;        // a full completion list stops the instance
    if (fin) {
        const int d = b * 2 * W + n_done + __popcll(m_fin & below);         // n_done < W, n_fin <= W
        s.done_rec[d] = t * s.B * W + p.h;
        s.done_score[d] = score;
    }
    return p;
}

// The attention rows of this step's live slots (the alpha of the step that chose the selections); `width` columns.
__device__ __forceinline__ void beam_copy_attention(float* hist_attn, const float* alpha, int base, int live, int width,
                                                    int lane) {
    if (!hist_attn) return;
    for (int e = lane; e < live * width; e += BEAM_WAVE) {
        const int r = e / width, c = e - r * width;
        hist_attn[(size_t)(base + r) * width + c] = alpha[(size_t)(base + r) * width + c];
    }
}

// The end of a step: the slots behind the continuing ones are dead (no parent = zero h / c, score 0; the kernel adds
// what else a dead slot of its own needs), and lane 0 moves the instance on.
template <class S>
__device__ __forceinline__ void beam_close(const S& s, int32_t* inst, int base, int lane, int t, const BeamPlace& p) {
    if (lane >= p.live_next && lane < s.beam_size) {
        s.parent[base + lane] = -1;
        s.score[base + lane] = 0.f;
    }
    if (lane == 0) {
        inst[0] = p.live_next;
        inst[1] = p.done_after;
        inst[2] = t + 1;
        if (p.live_next > 0) atomicAdd(s.live_total + t, p.live_next);
    }
}

__global__ __launch_bounds__(BEAM_WAVE) void speaker_beam_select_kernel(sf_spk_beam s, const int32_t* top_w,
                                                                        const float* top_lp, const float* alpha) {
    __shared__ int s_row[BEAM_WAVE], s_rank[BEAM_WAVE];
    __shared__ float s_score[BEAM_WAVE];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int W = s.beam_size, k = s.k, base = b * W;
    int32_t* inst = s.inst + 3 * b;
    const int live = inst[0], n_done = inst[1], t = inst[2];
    if (live <= 0 || t >= s.T) return;                  // ended instance (or steps issued past the end): no change
    const size_t hist = (size_t)t * (size_t)s.ld_hist;

    // ---- selection: every rank of a live slot is a successor
    const float my_score = lane < live ? s.score[base + lane] : 0.f;
    const int nsel = beam_merge(lane, live, W, k, my_score, top_lp + (size_t)(base + lane) * k,
                                [](int) { return true; }, s_row, s_rank, s_score);

    // ---- finals: EOS or the last word step (speaker.py:281-290)
    const bool sel = lane < nsel;
    const int prow = sel ? s_row[lane] : 0;
    const float score = sel ? s_score[lane] : 0.f;
    const int word = sel ? top_w[(size_t)(base + prow) * k + s_rank[lane]] : 0;
    const bool fin = sel && (word == s.eos || t == s.T - 1);
    const BeamPlace p = beam_place(s, b, lane, t, n_done, sel, fin, score);
    if (sel) {
        s.hist_word[hist + p.h] = word;
        s.hist_parent[hist + p.h] = base + prow;
        s.hist_score[hist + p.h] = score;
    }
    beam_copy_attention(s.hist_attn ? s.hist_attn + hist : nullptr, alpha, base, live, s.Tp, lane);

    // ---- the next step's slots (slot p of the next step is history position base + p of this step: the backchain
    // needs no other map)
    if (sel && !fin && p.live_next > 0) {
        s.words[p.h] = (int64_t)word;
        s.parent[p.h] = base + prow;
        s.score[p.h] = score;
    }
    // (dead slots are decoded and ignored: a valid word id)
    if (lane >= p.live_next && lane < W) s.words[base + lane] = (int64_t)s.eos;
    beam_close(s, inst, base, lane, t, p);
}

// The follower's step.  A slot's state is (row, view) of the navigation table, sid = row * V + view; a successor list
// ends at the first rank that is no candidate of the state (an action >= a_num -- sf_logprob_topk returns the masked
// columns as (column, -inf) behind the valid ones -- or a negative action: the is_valid filter of follower.py:626), so
// every list stays sorted and the merge applies unchanged.
__global__ __launch_bounds__(BEAM_WAVE) void follower_beam_select_kernel(sf_fol_beam s, const int32_t* top_a,
                                                                         const float* top_lp, const float* alpha) {
    __shared__ int s_row[BEAM_WAVE], s_rank[BEAM_WAVE], s_sid[BEAM_WAVE];
    __shared__ float s_score[BEAM_WAVE];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int W = s.beam_size, k = s.k, R = s.B * W, base = b * W;
    const int A = s.nav.A, V = s.nav.V;
    int32_t* inst = s.inst + 3 * b;
    const int live = inst[0], n_done = inst[1], t = inst[2];
    if (live <= 0 || t >= s.episode_len) return;        // ended instance (or steps issued past the end): no change
    const size_t hist = (size_t)t * (size_t)s.ld_hist;

    // ---- selection: a rank is a successor while its action is a candidate of the slot's state
    const int32_t* my_a = top_a + (size_t)(base + lane) * k;
    float my_score = 0.f;
    int my_anum = 0;
    if (lane < live) {
        const int sid = s.row[base + lane] * V + s.view[base + lane];
        s_sid[lane] = sid;
        my_score = s.score[base + lane];
        my_anum = s.nav.a_num[sid];
    }
    const int nsel = beam_merge(lane, live, W, k, my_score, top_lp + (size_t)(base + lane) * k,
                                [&](int j) { return my_a[j] >= 0 && my_a[j] < my_anum; }, s_row, s_rank, s_score);

    // ---- successor states (StateSpace.successors); finals: stop, or the last step (follower.py:674)
    const bool sel = lane < nsel;
    const int prow = sel ? s_row[lane] : 0;
    const float score = sel ? s_score[lane] : 0.f;
    const int act = sel ? top_a[(size_t)(base + prow) * k + s_rank[lane]] : 0;
    const int psid = sel ? s_sid[prow] : 0;
    int nsid = psid;
    if (sel && act != 0) {
        const int nxt = s.nav.next_row[(size_t)psid * A + act];
        if (nxt != psid / V) nsid = nxt * V + s.nav.cand_view[(size_t)psid * A + act];
    }
    const bool fin = sel && (act == 0 || t == s.episode_len - 1);
    const BeamPlace p = beam_place(s, b, lane, t, n_done, sel, fin, score);
    if (sel) {
        s.hist_parent[hist + p.h] = base + prow;
        s.hist_action[hist + p.h] = act;
        s.hist_rank[hist + p.h] = lane;
        s.hist_sid[hist + p.h] = nsid;
        s.hist_psid[hist + p.h] = psid;
        s.hist_score[hist + p.h] = score;
    }
    beam_copy_attention(s.hist_attn ? s.hist_attn + hist : nullptr, alpha, base, live, s.T, lane);

    // ---- the next step's slots (slot p of the next step is history position base + p of this step; every read of
    // row / view / score above happened before the merge's barrier)
    if (sel && !fin && p.live_next > 0) {
        s.row[p.h] = nsid / V;
        s.view[p.h] = nsid % V;
        s.row[R + p.h] = psid / V;                       // the parent's state and the action: the previous action's
        s.view[R + p.h] = psid % V;                      // embedding is looked up from them (sf_gather_actions_ld)
        s.act[p.h] = act;
        s.parent[p.h] = base + prow;
        s.score[p.h] = score;
    }
    // (dead slots are decoded and ignored: a zero embedding; row / view keep a valid state)
    if (lane >= p.live_next && lane < W) s.act[base + lane] = 0;
    beam_close(s, inst, base, lane, t, p);
}

// ---- the state-factored search (reference: Seq2SeqAgent.state_factored_search, tasks/R2R/follower.py:783-905;
// sim/frontier_core.cpp: advance_raw + fill_inputs_raw; search.DeviceStateFactored), layout contract:
// include/sf_hip.h, sf_state_factored_select.
//
// One workgroup per instance.  The instance's successors (frontier column r, action a: index g = r * A + a, the
// generation order) sit in LDS; the reference's stable descending sort is a rank -- the number of successors that come
// before g -- counted by g's own lane, and so are "first of its (key, final) group", the number of new nodes before a
// new node and of new slots before a new slot: every lane decides for its own successors, nothing is ordered by
// arrival.  Distinct groups touch distinct dictionary entries, so the entries are checked and replaced in parallel.
constexpr int SFS_THREADS = 256;        // 4 wavefronts
constexpr int SFS_MAX_SUCC = 1024;      // successor_size * A
constexpr int SFS_MAX_S = 64;           // successor_size
constexpr int SFS_MAX_B = SFS_THREADS;  // one lane per instance in the pack launch

// ordering key of a score: a NaN sorts last, the order stays total
__device__ __forceinline__ float sfs_ordkey(float x) { return x != x ? -INFINITY : x; }

// First maximum above -inf over the workgroup: every lane brings the first maximum (v, i) of its own strided scan
// (i = -1: none); every lane gets the greatest v, the lowest i among equals.  sv / si: 4 words of LDS each.
__device__ __forceinline__ int sfs_first_max(float& v, int i, float* sv, int* si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
            v = ov;
            i = oi;
        }
    }
    __syncthreads();                                      // (the scratch words of the previous call have been read)
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = v;
        si[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    v = sv[0];
    i = si[0];
#pragma unroll
    for (int w = 1; w < SFS_THREADS / 64; ++w) {
        const float ov = sv[w];
        const int oi = si[w];
        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
            v = ov;
            i = oi;
        }
    }
    return i;
}

__global__ __launch_bounds__(SFS_THREADS) void state_factored_select_kernel(sf_state_search s, const float* logp,
                                                                            int ld) {
    __shared__ float s_score[SFS_MAX_SUCC];
    __shared__ int s_key[SFS_MAX_SUCC], s_nsid[SFS_MAX_SUCC], s_rank[SFS_MAX_SUCC], s_flag[SFS_MAX_SUCC];
    __shared__ int s_win[SFS_MAX_SUCC], s_slot[SFS_MAX_SUCC];
    __shared__ int s_f[SFS_MAX_S], s_fsid[SFS_MAX_S], s_fkey[SFS_MAX_S], s_fcount[SFS_MAX_S], s_fstart[SFS_MAX_S];
    __shared__ int s_fna[SFS_MAX_S];
    __shared__ float s_fscore[SFS_MAX_S];
    __shared__ int s_cnt[4];                              // new nodes, new open slots, new held slots, bad key
    __shared__ float s_rv[SFS_THREADS / 64];
    __shared__ int s_ri[SFS_THREADS / 64];
    __shared__ int s_pk[SFS_MAX_S], s_pn[SFS_MAX_S], s_ph[SFS_MAX_S];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (s.status[0] <= 0 || s.status[3] != 0) return;    // an empty frontier, or an overflow: no change
    int32_t* in = s.inst + 8 * b;
    int n_nodes = in[0], n_open = in[1], n_held = in[2];
    const int n_comp = in[3], n_vis = in[4], first = in[6];
    const int nf = min(max(in[5], 0), s.successor_size);
    if (n_comp >= s.completion_size) return;             // it has its completions
    const int A = s.nav.A, V = s.nav.V, S = s.successor_size, K = s.n_keys;
    const int base = s.status[1], born = s.status[2] + 1;
    const size_t kb = (size_t)b * K, sb = (size_t)b * s.slot_cap;
    const int node0 = b * s.node_cap;

    // ---- the frontier's nodes
    if (tid < 4) s_cnt[tid] = 0;
    if (tid < nf) {
        const int f = s.frontier[b * S + tid];
        const int sid = s.node_sid[f];
        s_f[tid] = f;
        s_fsid[tid] = sid;
        s_fkey[tid] = s.node_key[f];
        s_fcount[tid] = s.node_count[f];
        s_fstart[tid] = s.node_start[f];
        s_fscore[tid] = s.node_score[f];
        s_fna[tid] = min(s.nav.a_num[sid], A);
    }
    __syncthreads();

    // ---- successors in generation order
    const int M = nf * A;
    for (int g = tid; g < M; g += SFS_THREADS) {
        const int r = g / A, a = g - r * A;
        int flag = 0, key = 0, nsid = 0;
        float score = 0.f;
        if (a < s_fna[r]) {
            const int st = s_fsid[r];
            const int nxt = s.nav.next_row[(size_t)st * A + a];
            const bool stay = a == 0 || nxt == st / V;                       // env.py:126-146
            nsid = stay ? st : nxt * V + s.nav.cand_view[(size_t)st * A + a];
            if (stay) {
                key = s_fkey[r];
            } else {                                                         // follower.py:722, 843: world_state[0:n]
                const int local_row = nsid / V - s.base_row[b];
                key = s.key_fields == 4 ? local_row * V + nsid % V
                    : s.key_fields == 3 ? local_row * 12 + nsid % 12
                    : s.key_fields == 2 ? local_row : 0;
            }
            const bool fin = a == 0 || s_fcount[r] + 1 == s.episode_len;
            score = s_fscore[r] + logp[(size_t)(first + r) * ld + a];        // float32 add (follower.py:826)
            flag = 1 | (fin ? 2 : 0) | (stay ? 4 : 0);
            if (key < 0 || key >= K) atomicOr(&s_cnt[3], 1);
        }
        s_flag[g] = flag;
        s_key[g] = key;
        s_nsid[g] = nsid;
        s_score[g] = score;
    }
    __syncthreads();
    if (s_cnt[3]) {
        if (tid == 0) in[7] |= SF_SEARCH_OVF_KEY;
        return;
    }

    // ---- rank in the stable descending sort; is it the first of its (key, final) group
    for (int g = tid; g < M; g += SFS_THREADS) {
        const int fg = s_flag[g];
        int rank = -1, win = 0;
        if (fg & 1) {
            const float kg = sfs_ordkey(s_score[g]);
            const int key = s_key[g];
            bool lead = true;
            rank = 0;
            for (int h = 0; h < M; ++h) {
                const int fh = s_flag[h];
                if (!(fh & 1)) continue;
                const float kh = sfs_ordkey(s_score[h]);
                if (kh > kg || (kh == kg && h < g)) {
                    ++rank;
                    if (s_key[h] == key && !((fh ^ fg) & 2)) lead = false;   // a better one came first
                }
            }
            // ---- it enters if its dictionary holds nothing for the key, or a strictly smaller score
            if (lead) {
                const bool fin = fg & 2;
                const int slot = (fin ? s.held_slot : s.open_slot)[kb + key];
                s_slot[g] = slot;
                if (slot < 0) {
                    win = 2;
                } else {
                    const int cur = (fin ? s.held_node : s.open_node)[sb + slot];
                    win = s.node_score[cur] < s_score[g] ? 1 : 0;
                }
                if (win) atomicAdd(&s_cnt[0], 1);
                if (win == 2) atomicAdd(&s_cnt[fin ? 2 : 1], 1);
            }
        }
        s_rank[g] = rank;
        s_win[g] = win;
    }
    __syncthreads();
    const int n_new = s_cnt[0], new_open = s_cnt[1], new_held = s_cnt[2];
    {
        int ovf = 0;
        if (n_nodes + n_new > s.node_cap) ovf |= SF_SEARCH_OVF_NODES;
        if (n_open + new_open > s.slot_cap || n_held + new_held > s.slot_cap) ovf |= SF_SEARCH_OVF_SLOTS;
        if (ovf) {                                        // nothing of this iteration is written
            if (tid == 0) in[7] |= ovf;
            return;
        }
    }

    // ---- the new nodes and their entries, numbered in processing order
    for (int g = tid; g < M; g += SFS_THREADS) {
        const int win = s_win[g];
        if (!win) continue;
        const int fg = s_flag[g], rank = s_rank[g];
        const bool fin = fg & 2;
        int before = 0, slots_before = 0;
        for (int h = 0; h < M; ++h) {
            const int wh = s_win[h];
            if (wh && s_rank[h] < rank) {
                ++before;
                if (wh == 2 && !((s_flag[h] ^ fg) & 2)) ++slots_before;
            }
        }
        const int r = g / A, a = g - r * A;
        const int id = node0 + n_nodes + before;
        s.node_parent[id] = s_f[r];
        s.node_sid[id] = s_nsid[g];
        s.node_key[id] = s_key[g];
        s.node_action[id] = a;
        s.node_count[id] = s_fcount[r] + 1;
        s.node_pool[id] = base + first + r;
        s.node_start[id] = (s_fstart[r] && (fg & 4)) ? 1 : 0;
        s.node_born[id] = born;
        s.node_score[id] = s_score[g];
        int slot = s_slot[g];
        if (win == 2) {
            slot = (fin ? n_held : n_open) + slots_before;
            (fin ? s.held_slot : s.open_slot)[kb + s_key[g]] = slot;
            (fin ? s.held_key : s.open_key)[sb + slot] = s_key[g];
        }
        (fin ? s.held_node : s.open_node)[sb + slot] = id;
        (fin ? s.held_pick : s.open_pick)[sb + slot] = s_score[g];
    }
    n_nodes += n_new;
    n_open += new_open;
    n_held += new_held;
    __syncthreads();

    // ---- the `successor_size` best entries not expanded yet (heapq.nlargest over chain(cache, holding),
    // follower.py:861-865: equal scores go to the state to expand, then to the older entry)
    int n_picks = 0;
    for (; n_picks < S; ++n_picks) {
        float mo = -INFINITY, mh = -INFINITY;
        int ao = -1, ah = -1;
        for (int i = tid; i < n_open; i += SFS_THREADS) {
            const float p = s.open_pick[sb + i];
            if (p > mo) {
                mo = p;
                ao = i;
            }
        }
        for (int i = tid; i < n_held; i += SFS_THREADS) {
            const float p = s.held_pick[sb + i];
            if (p > mh) {
                mh = p;
                ah = i;
            }
        }
        ao = sfs_first_max(mo, ao, s_rv, s_ri);
        ah = sfs_first_max(mh, ah, s_rv, s_ri);
        if (ao < 0 && ah < 0) break;
        const bool use_h = ah >= 0 && (ao < 0 || mh > mo);
        if (tid == 0) {
            const int slot = use_h ? ah : ao;
            (use_h ? s.held_pick : s.open_pick)[sb + slot] = -INFINITY;     // expanded
            s_pk[n_picks] = (use_h ? s.held_key : s.open_key)[sb + slot];
            s_pn[n_picks] = (use_h ? s.held_node : s.open_node)[sb + slot];
            s_ph[n_picks] = use_h;
        }
        __syncthreads();
    }

    // ---- completions, the next frontier, the visits
    if (tid == 0) {
        int nc = n_comp, nv = n_vis, cnt = 0, ovf = 0;
        const int comp_cap = s.completion_size + S;
        for (int p = 0; p < n_picks; ++p) {
            if (!s_ph[p]) continue;
            const int key = s_pk[p], node = s_pn[p];
            const int old = s.comp_node[kb + key];
            if (old < 0) {
                s.comp_node[kb + key] = node;
                if (nc < comp_cap) s.comp_order[(size_t)b * comp_cap + nc] = key;
                ++nc;
            } else if (s.node_score[old] < s.node_score[node]) {
                s.comp_node[kb + key] = node;
            }
        }
        for (int p = 0; p < n_picks; ++p) {
            if (s_ph[p] || nc >= s.completion_size) continue;
            if (nv >= s.visit_cap) {
                ovf = SF_SEARCH_OVF_VISITS;
                break;
            }
            s.frontier[b * S + cnt++] = s_pn[p];
            s.visits[(size_t)b * s.visit_cap + nv++] = s_pn[p];
        }
        in[0] = n_nodes;
        in[1] = n_open;
        in[2] = n_held;
        in[3] = nc;
        in[4] = nv;
        in[5] = cnt;
        if (ovf) in[7] |= ovf;
    }
}

// Column i of the decoder step's [8, cap] input block for node f (frontier_core.cpp: fill_inputs_raw).
__device__ __forceinline__ void sfs_write_column(const sf_state_search& s, int32_t* o, int i, int f, int dst) {
    const int cap = s.cap, V = s.nav.V;
    const int sid = s.node_sid[f], p = s.node_parent[f];
    const int ps = p >= 0 ? s.node_sid[p] : sid;
    o[0 * cap + i] = sid / V;
    o[1 * cap + i] = ps / V;
    o[2 * cap + i] = sid % V;
    o[3 * cap + i] = ps % V;
    o[4 * cap + i] = p >= 0 ? s.node_action[f] : 0;
    o[5 * cap + i] = s.node_pool[f];
    o[6 * cap + i] = f / s.node_cap;
    o[7 * cap + i] = dst;
}

// The second launch: one workgroup, lane b = instance b.  Prefix sum of the instances' frontier counts, the overflow
// flags, base, and the next input block.
__global__ __launch_bounds__(SFS_THREADS) void state_factored_pack_kernel(sf_state_search s, int32_t* dev_in) {
    __shared__ int s_sum[SFS_THREADS];
    __shared__ int s_flags, s_head;
    const int tid = threadIdx.x, B = s.B, S = s.successor_size;
    const int n_old = s.status[0], base_old = s.status[1], iters = s.status[2];
    if (n_old <= 0 || s.status[3] != 0) return;          // an empty frontier, or an overflow: no change
    int cnt = 0, fl = 0;
    if (tid < B) {
        cnt = min(max(s.inst[8 * tid + 5], 0), S);
        fl = s.inst[8 * tid + 7];
    }
    s_sum[tid] = cnt;
    if (tid == 0) {
        s_flags = 0;
        s_head = 0;                                       // instance 0's root
    }
    __syncthreads();
    if (fl) atomicOr(&s_flags, fl);
    for (int d = 1; d < SFS_THREADS; d <<= 1) {
        const int v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    const int first = s_sum[tid] - cnt;
    int N = s_sum[SFS_THREADS - 1];
    const int base = base_old + n_old;
    int flags = s_flags;
    if (!flags && N > 0 && base + N > s.pool_rows) flags = SF_SEARCH_OVF_POOL;
    if (flags) {                                          // the frontier is emptied
        N = 0;
        cnt = 0;
    }
    if (tid < B) {
        s.inst[8 * tid + 5] = cnt;
        s.inst[8 * tid + 6] = first;
    }
    if (cnt > 0 && first == 0) s_head = s.frontier[tid * S];                 // (one lane: the owner of column 0)
    __syncthreads();
    for (int j = 0; j < cnt; ++j) sfs_write_column(s, dev_in, first + j, s.frontier[tid * S + j], base + first + j);
    const int head = s_head;
    for (int i = N + tid; i < s.cap; i += SFS_THREADS) sfs_write_column(s, dev_in, i, head, -1);
    if (tid == 0) {
        s.status[0] = N;
        s.status[1] = base;
        s.status[2] = iters + 1;
        s.status[3] = flags;
    }
}

}  // namespace

bool state_factored_select_supported(const sf_state_search& s) {
    return (int64_t)s.successor_size * s.nav.A <= SFS_MAX_SUCC && s.successor_size <= SFS_MAX_S && s.B <= SFS_MAX_B;
}

int state_factored_select(const sf_state_search& s, const float* logp, int ld_logp, int32_t* dev_in, hipStream_t st) {
    if (!state_factored_select_supported(s)) return SF_ERR_UNSUPPORTED;
    SF_LAUNCH(state_factored_select_kernel, dim3(s.B), dim3(SFS_THREADS), 0, st, s, logp, ld_logp);
    SF_LAUNCH(state_factored_pack_kernel, dim3(1), dim3(SFS_THREADS), 0, st, s, dev_in);
    return launch_status();
}

int speaker_beam_select(const sf_spk_beam& s, const int32_t* top_w, const float* top_lp, const float* alpha,
                        hipStream_t st) {
    if (s.beam_size > 64) return SF_ERR_UNSUPPORTED;
    SF_LAUNCH(speaker_beam_select_kernel, dim3(s.B), dim3(BEAM_WAVE), 0, st, s, top_w, top_lp, alpha);
    return launch_status();
}

int follower_beam_select(const sf_fol_beam& s, const int32_t* top_a, const float* top_lp, const float* alpha,
                         hipStream_t st) {
    if (s.beam_size > 64) return SF_ERR_UNSUPPORTED;
    SF_LAUNCH(follower_beam_select_kernel, dim3(s.B), dim3(BEAM_WAVE), 0, st, s, top_a, top_lp, alpha);
    return launch_status();
}

}  // namespace sf
