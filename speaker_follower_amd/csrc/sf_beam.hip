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
#include "sf_kernels.h"

namespace sf {
namespace {

constexpr int BEAM_WAVE = 64;           // one lane per slot: beam_size <= 64

// (score, flat) of `o` comes before (score, flat) of the current best: higher score, then lower flat index.
// An empty head is (-inf, INT_MAX): every real candidate, a -inf one included, comes before it.
__device__ __forceinline__ bool beam_before(float os, int of, float bs, int bf) {
    return os > bs || (os == bs && of < bf);
}

__global__ __launch_bounds__(BEAM_WAVE) void speaker_beam_select_kernel(sf_spk_beam s, const int32_t* top_w,
                                                                        const float* top_lp, const float* alpha) {
    __shared__ int s_row[BEAM_WAVE], s_word[BEAM_WAVE];
    __shared__ float s_score[BEAM_WAVE];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int W = s.beam_size, k = s.k, R = s.B * W, base = b * W;
    int32_t* inst = s.inst + 3 * b;
    const int live = inst[0], n_done = inst[1], t = inst[2];
    if (live <= 0 || t >= s.T) return;                  // ended instance (or steps issued past the end): no change
    const size_t hist = (size_t)t * (size_t)s.ld_hist;

    // ---- selection: merge of the live slots' sorted successor lists
    const int32_t* my_w = top_w + (size_t)(base + lane) * k;
    const float* my_lp = top_lp + (size_t)(base + lane) * k;
    const float my_score = lane < live ? s.score[base + lane] : 0.f;
    int j = 0;
    float head = -INFINITY;                               // the head's score (float32 add, as speaker.py:277)
    int head_flat = 0x7fffffff;
    if (lane < live) {
        head = my_score + my_lp[0];
        head_flat = lane * k;
    }
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
        if (bf == 0x7fffffff) break;                      // every list is exhausted (live * k < beam_size)
        if (bf == head_flat) {                            // this lane's head won: record it, advance the list
            s_row[nsel] = lane;
            s_word[nsel] = my_w[j];
            s_score[nsel] = head;
            ++j;
            if (j < k) {
                head = my_score + my_lp[j];
                head_flat = lane * k + j;
            } else {
                head = -INFINITY;
                head_flat = 0x7fffffff;
            }
        }
    }
    __syncthreads();

    // ---- finals (EOS or the last word step) after the continuing hypotheses, both in selection order
    const bool sel = lane < nsel;
    const int word = sel ? s_word[lane] : 0;
    const bool fin = sel && (word == s.eos || t == s.T - 1);
    const unsigned long long m_fin = __ballot(fin), m_cont = __ballot(sel && !fin);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_fin = __popcll(m_fin), n_cont = __popcll(m_cont);
    const int pos = fin ? n_cont + __popcll(m_fin & below) : __popcll(m_cont & below);
    const int done_after = n_done + n_fin;
    const int live_next = done_after >= W ? 0 : n_cont;  // speaker.py:281-290: a full completion list stops the path
    if (sel) {
        const int h = base + pos;
        s.hist_word[hist + h] = word;
        s.hist_parent[hist + h] = base + s_row[lane];
        s.hist_score[hist + h] = s_score[lane];
        if (fin) {
            const int d = b * 2 * W + n_done + __popcll(m_fin & below);     // n_done < W, n_fin <= W
            s.done_rec[d] = t * R + h;
            s.done_score[d] = s_score[lane];
        }
    }
    // the attention rows of this step's live slots (the alpha of the step that chose the new words)
    if (s.hist_attn) {
        const int Tp = s.Tp;
        for (int e = lane; e < live * Tp; e += BEAM_WAVE) {
            const int r = e / Tp, c = e - r * Tp;
            s.hist_attn[hist + (size_t)(base + r) * Tp + c] = alpha[(size_t)(base + r) * Tp + c];
        }
    }

    // ---- the next step's slots: continuing hypotheses compacted to the front in selection order, the rest dead
    // (slot p of the next step is history position base + p of this step: the backchain needs no other map)
    if (sel && !fin && live_next > 0) {
        s.words[base + pos] = (int64_t)word;
        s.parent[base + pos] = base + s_row[lane];
        s.score[base + pos] = s_score[lane];
    }
    if (lane >= live_next && lane < W) {
        s.words[base + lane] = (int64_t)s.eos;           // (a valid word id: dead slots are decoded and ignored)
        s.parent[base + lane] = -1;                      // (zero h / c)
        s.score[base + lane] = 0.f;
    }
    if (lane == 0) {
        inst[0] = live_next;
        inst[1] = done_after;
        inst[2] = t + 1;
        if (live_next > 0) atomicAdd(s.live_total + t, live_next);
    }
}

// The follower's step.  A slot's state is (row, view) of the navigation table, sid = row * V + view; a successor list
// ends at the first rank that is no candidate of the state (an action >= a_num -- sf_logprob_topk returns the masked
// columns as (column, -inf) behind the valid ones -- or a negative action: the is_valid filter of follower.py:626), so
// every list stays sorted and the merge above applies unchanged.
__global__ __launch_bounds__(BEAM_WAVE) void follower_beam_select_kernel(sf_fol_beam s, const int32_t* top_a,
                                                                         const float* top_lp, const float* alpha) {
    __shared__ int s_row[BEAM_WAVE], s_act[BEAM_WAVE], s_sid[BEAM_WAVE];
    __shared__ float s_score[BEAM_WAVE];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int W = s.beam_size, k = s.k, R = s.B * W, base = b * W;
    const int A = s.nav.A, V = s.nav.V;
    int32_t* inst = s.inst + 3 * b;
    const int live = inst[0], n_done = inst[1], t = inst[2];
    if (live <= 0 || t >= s.episode_len) return;        // ended instance (or steps issued past the end): no change
    const size_t hist = (size_t)t * (size_t)s.ld_hist;

    // ---- selection: merge of the live slots' sorted successor lists
    const int32_t* my_a = top_a + (size_t)(base + lane) * k;
    const float* my_lp = top_lp + (size_t)(base + lane) * k;
    float my_score = 0.f;
    int my_anum = 0;
    if (lane < live) {
        const int sid = s.row[base + lane] * V + s.view[base + lane];
        s_sid[lane] = sid;
        my_score = s.score[base + lane];
        my_anum = s.nav.a_num[sid];
    }
    int j = 0;
    float head = -INFINITY;                               // the head's score (float32 add, as follower.py:629)
    int head_flat = 0x7fffffff, head_act = -1;
    if (lane < live) {
        head_act = my_a[0];
        if (head_act >= 0 && head_act < my_anum) {
            head = my_score + my_lp[0];
            head_flat = lane * k;
        }
    }
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
            s_act[nsel] = head_act;
            s_score[nsel] = head;
            ++j;
            head = -INFINITY;
            head_flat = 0x7fffffff;
            if (j < k) {
                head_act = my_a[j];
                if (head_act >= 0 && head_act < my_anum) {
                    head = my_score + my_lp[j];
                    head_flat = lane * k + j;
                }
            }
        }
    }
    __syncthreads();

    // ---- successor states (StateSpace.successors) and finals (stop, or the last step), both in selection order
    const bool sel = lane < nsel;
    const int prow = sel ? s_row[lane] : 0, act = sel ? s_act[lane] : 0;
    const int psid = sel ? s_sid[prow] : 0;
    int nsid = psid;
    if (sel && act != 0) {
        const int nxt = s.nav.next_row[(size_t)psid * A + act];
        if (nxt != psid / V) nsid = nxt * V + s.nav.cand_view[(size_t)psid * A + act];
    }
    const bool fin = sel && (act == 0 || t == s.episode_len - 1);
    const unsigned long long m_fin = __ballot(fin), m_cont = __ballot(sel && !fin);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_fin = __popcll(m_fin), n_cont = __popcll(m_cont);
    const int pos = fin ? n_cont + __popcll(m_fin & below) : __popcll(m_cont & below);
    const int done_after = n_done + n_fin;
    const int live_next = done_after >= W ? 0 : n_cont;  // follower.py:674: a full completion list stops the instance
    if (sel) {
        const int h = base + pos;
        s.hist_parent[hist + h] = base + prow;
        s.hist_action[hist + h] = act;
        s.hist_rank[hist + h] = lane;
        s.hist_sid[hist + h] = nsid;
        s.hist_psid[hist + h] = psid;
        s.hist_score[hist + h] = s_score[lane];
        if (fin) {
            const int d = b * 2 * W + n_done + __popcll(m_fin & below);     // n_done < W, n_fin <= W
            s.done_rec[d] = t * R + h;
            s.done_score[d] = s_score[lane];
        }
    }
    // the attention rows of this step's live slots (the alpha of the step that chose the actions)
    if (s.hist_attn) {
        const int T = s.T;
        for (int e = lane; e < live * T; e += BEAM_WAVE) {
            const int r = e / T, c = e - r * T;
            s.hist_attn[hist + (size_t)(base + r) * T + c] = alpha[(size_t)(base + r) * T + c];
        }
    }

    // ---- the next step's slots: continuing hypotheses compacted to the front in selection order, the rest dead
    // (slot p of the next step is history position base + p of this step; every read of row / view / score above
    // happened before the barrier)
    if (sel && !fin && live_next > 0) {
        s.row[base + pos] = nsid / V;
        s.view[base + pos] = nsid % V;
        s.row[R + base + pos] = psid / V;                // the parent's state and the action: the previous action's
        s.view[R + base + pos] = psid % V;               // embedding is looked up from them (sf_gather_actions_ld)
        s.act[base + pos] = act;
        s.parent[base + pos] = base + prow;
        s.score[base + pos] = s_score[lane];
    }
    if (lane >= live_next && lane < W) {
        s.act[base + lane] = 0;                          // (zero embedding; row / view keep a valid state: dead slots
        s.parent[base + lane] = -1;                      // are decoded and ignored)
        s.score[base + lane] = 0.f;
    }
    if (lane == 0) {
        inst[0] = live_next;
        inst[1] = done_after;
        inst[2] = t + 1;
        if (live_next > 0) atomicAdd(s.live_total + t, live_next);
    }
}

}  // namespace

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
