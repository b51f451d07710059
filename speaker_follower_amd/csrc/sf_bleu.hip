// Corpus BLEU counted on the device (reference: tasks/R2R/eval_speaker.py:11-122, tasks/R2R/bleu.py:15-72 and the
// multi-bleu script bleu.py pipes its files through; speaker_follower_amd/speaker_evaluation.py restates them and
// bleu_count_rows there is the specification of this kernel).  Per hypothesis ten integers: clipped n-gram matches and
// n-gram totals for n = 1..4, the hypothesis length, the length of the closest reference.  Integers only: the one
// place floating point happens is speaker_evaluation.bleu_from_counts, on the host, over the ten sums.
//
// Words are ids of an evaluation-private dictionary of at most 2^16 entries, so an n-gram IS the packing of its up to
// four 16-bit ids into one 64-bit key: one compare per pair of n-grams, no hashing, nothing can collide.  n-grams of
// different orders are never compared with each other (each order has its own mask and its own counters).
#include "sf_common.h"

#include <atomic>

namespace sf {
namespace {

std::atomic<int> g_bleu_max_dict{SF_BLEU_MAX_DICT};
std::atomic<int> g_bleu_max_hyp{SF_BLEU_MAX_HYP};
std::atomic<int> g_bleu_max_ref{SF_BLEU_MAX_REF};
std::atomic<int> g_bleu_max_refs{SF_BLEU_MAX_REFS};

constexpr int PAD_WORDS = 4;                    // behind every staged sentence: the rolling key reads w[j + 4]

__device__ __forceinline__ uint64_t key_at(const uint16_t* w, int j) {
    return (uint64_t)w[j] | ((uint64_t)w[j + 1] << 16) | ((uint64_t)w[j + 2] << 32) | ((uint64_t)w[j + 3] << 48);
}

// Occurrences of the n-grams that start with the words of `ki` among the n-grams of w[0..L): cnt[n-1] += 1 for every
// start j with j + n <= L whose first n words equal the first n words of ki; before[n-1] is raised when such a j lies
// below `upto`.  One pass serves all four orders: the key of start j + 1 is the key of start j shifted by one word.
// L is uniform over the wave, every lane reads the same LDS word (a broadcast).
__device__ __forceinline__ void count_matches(const uint16_t* w, int L, uint64_t ki, int upto, int cnt[4], int before[4]) {
    if (L <= 0) return;
    uint64_t k = key_at(w, 0);
    for (int j = 0; j < L; ++j) {
        const uint64_t x = k ^ ki;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const uint64_t mask = n == 3 ? ~0ull : ((1ull << (16 * (n + 1))) - 1);
            const int eq = (x & mask) == 0 && j + n < L;
            cnt[n] += eq;
            before[n] |= eq && j < upto;
        }
        k = (k >> 16) | ((uint64_t)w[j + PAD_WORDS] << 48);
    }
}

__device__ __forceinline__ int64_t word_at(const sf_bleu_batch& p, int s, int b) {
    const int64_t at = (int64_t)s * p.n_hyps + b;
    return p.word_bytes == 8 ? ((const int64_t*)p.words)[at] : (int64_t)((const int16_t*)p.words)[at];
}

// One wavefront (= one workgroup) per hypothesis; lane l owns the hypothesis start positions l, l + 64, ...
__global__ __launch_bounds__(WAVE) void bleu_counts_kernel(sf_bleu_batch p, int lim_hyp, int lim_ref,
                                                           int32_t* __restrict__ err) {
    __shared__ uint16_t hyp[SF_BLEU_MAX_HYP + PAD_WORDS];
    __shared__ uint16_t ref[SF_BLEU_MAX_REFS][SF_BLEU_MAX_REF + PAD_WORDS];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= p.n_hyps) return;
    const int slot = p.slot[b];                                 // (uniform over the wave, as every return below)
    if (slot == -1) return;
    if (slot < -1 || slot >= p.n_slots) {
        if (lane == 0) *err = 1;
        return;
    }
    const int R = p.n_refs;
    int bad = 0, H = 0;
    if (p.words) {
        // column b up to, not including, its first EOS; all S words when there is none
        int first = p.S;
        for (int s = lane; s < p.S; s += WAVE)
            if (word_at(p, s, b) == p.eos) {
                first = s;
                break;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, WAVE));
        // a vocabulary word is no, one or two BLEU words (remap[w] = (-1, -1), (a, -1), (a, b)): a word's place in the
        // hypothesis is the number of BLEU words before it -- a prefix sum over each chunk of 64 positions
        int base = 0;
        for (int s0 = 0; s0 < first; s0 += WAVE) {
            const int s = s0 + lane;
            int id0 = -1, id1 = -1, len = 0;
            if (s < first) {
                const int64_t w = word_at(p, s, b);
                if (w >= 0 && w < p.n_vocab) {
                    id0 = p.remap[2 * w];
                    id1 = p.remap[2 * w + 1];
                    if (id0 == -1 && id1 == -1) len = 0;
                    else if ((unsigned)id0 < (unsigned)p.n_dict && id1 == -1) len = 1;
                    else if ((unsigned)id0 < (unsigned)p.n_dict && (unsigned)id1 < (unsigned)p.n_dict) len = 2;
                    else bad = 1;
                } else {
                    bad = 1;
                }
            }
            int upto = len;                                     // inclusive prefix sum over the lanes
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const int below = __shfl_up(upto, off, WAVE);
                if (lane >= off) upto += below;
            }
            const int at = base + upto - len;
            if (len >= 1 && at < lim_hyp) hyp[at] = (uint16_t)id0;
            if (len == 2 && at + 1 < lim_hyp) hyp[at + 1] = (uint16_t)id1;
            base += __shfl(upto, WAVE - 1, WAVE);
        }
        H = base;
        if (H > lim_hyp) {
            bad = 1;
            H = 0;
        }
    } else {
        const int o0 = p.hyp_off[b];
        H = p.hyp_off[b + 1] - o0;
        if (o0 < 0 || H < 0 || H > lim_hyp) {
            bad = 1;
            H = 0;
        } else {
            for (int s = lane; s < H; s += WAVE) {
                const int id = p.hyp_ids[o0 + s];
                if ((unsigned)id >= (unsigned)p.n_dict) bad = 1; else hyp[s] = (uint16_t)id;
            }
        }
    }
    int rl[SF_BLEU_MAX_REFS];
#pragma unroll
    for (int r = 0; r < SF_BLEU_MAX_REFS; ++r) {
        rl[r] = 0;
        if (r < R) {
            const int o0 = p.ref_off[(int64_t)slot * R + r];
            const int L = p.ref_off[(int64_t)slot * R + r + 1] - o0;
            if (o0 < 0 || L < 0 || L > lim_ref) {
                bad = 1;
            } else {
                rl[r] = L;
                for (int s = lane; s < L; s += WAVE) {
                    const int id = p.ref_ids[o0 + s];
                    if ((unsigned)id >= (unsigned)p.n_dict) bad = 1; else ref[r][s] = (uint16_t)id;
                }
                if (lane < PAD_WORDS) ref[r][L + lane] = 0;
            }
        }
    }
    if (!bad && lane < PAD_WORDS) hyp[H + lane] = 0;
    if (__syncthreads_or(bad)) {                                // anything inconsistent: nothing is written
        if (lane == 0) *err = 1;
        return;
    }
    int correct[4] = {0, 0, 0, 0};
    for (int i0 = 0; i0 < H; i0 += WAVE) {
        const int i = i0 + lane;
        const bool mine = i < H;
        const uint64_t ki = mine ? key_at(hyp, i) : 0;
        int in_hyp[4] = {0, 0, 0, 0}, before[4] = {0, 0, 0, 0}, in_refs[4] = {0, 0, 0, 0};
        count_matches(hyp, H, ki, i, in_hyp, before);
#pragma unroll
        for (int r = 0; r < SF_BLEU_MAX_REFS; ++r) {
            if (r < R) {
                int in_ref[4] = {0, 0, 0, 0}, unused[4] = {0, 0, 0, 0};
                count_matches(ref[r], rl[r], ki, 0, in_ref, unused);
#pragma unroll
                for (int n = 0; n < 4; ++n) in_refs[n] = max(in_refs[n], in_ref[n]);
            }
        }
        // a DISTINCT n-gram counts once: at its first start position in the hypothesis
#pragma unroll
        for (int n = 0; n < 4; ++n)
            if (mine && i + n < H && !before[n]) correct[n] += min(in_hyp[n], in_refs[n]);
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) correct[n] += __shfl_xor(correct[n], off, WAVE);
    // the reference closest in length, the SHORTER one on a tie (the script starts from 9999 / 9999)
    int closest_diff = 9999, closest = 9999;
#pragma unroll
    for (int r = 0; r < SF_BLEU_MAX_REFS; ++r) {
        if (r < R) {
            const int diff = abs(H - rl[r]);
            if (diff < closest_diff) {
                closest_diff = diff;
                closest = rl[r];
            } else if (diff == closest_diff && rl[r] < closest) {
                closest = rl[r];
            }
        }
    }
    if (lane < 10) {
        int v = closest;
        if (lane == 0) v = correct[0];
        else if (lane == 1) v = correct[1];
        else if (lane == 2) v = correct[2];
        else if (lane == 3) v = correct[3];
        else if (lane < 8) v = max(H - (lane - 4), 0);
        else if (lane == 8) v = H;
        p.rows[(int64_t)slot * 10 + lane] = v;
        atomicAdd((unsigned long long*)(p.sums + lane), (unsigned long long)v);
    }
}

}  // namespace
}  // namespace sf

extern "C" int sf_bleu_max_dict(void) { return sf::g_bleu_max_dict.load(); }
extern "C" int sf_bleu_max_hyp(void) { return sf::g_bleu_max_hyp.load(); }
extern "C" int sf_bleu_max_ref(void) { return sf::g_bleu_max_ref.load(); }
extern "C" int sf_bleu_max_refs(void) { return sf::g_bleu_max_refs.load(); }

extern "C" void sf_debug_bleu_limits(int max_dict, int max_hyp, int max_ref, int max_refs) {
    sf::g_bleu_max_dict.store(max_dict >= 1 && max_dict <= SF_BLEU_MAX_DICT ? max_dict : SF_BLEU_MAX_DICT);
    sf::g_bleu_max_hyp.store(max_hyp >= 1 && max_hyp <= SF_BLEU_MAX_HYP ? max_hyp : SF_BLEU_MAX_HYP);
    sf::g_bleu_max_ref.store(max_ref >= 1 && max_ref <= SF_BLEU_MAX_REF ? max_ref : SF_BLEU_MAX_REF);
    sf::g_bleu_max_refs.store(max_refs >= 1 && max_refs <= SF_BLEU_MAX_REFS ? max_refs : SF_BLEU_MAX_REFS);
}

extern "C" int sf_bleu_counts(const sf_bleu_batch* b, int32_t* err, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(b && err && b->n_hyps >= 1 && b->n_slots >= 1 && b->n_refs >= 1 && b->n_dict >= 1 && b->max_ref >= 0 &&
                 b->ref_ids && b->ref_off && b->slot && b->rows && b->sums);
    int max_hyp = b->max_hyp;
    if (b->words) {
        SF_CHECK_ARG(b->remap && b->S >= 1 && b->n_vocab >= 1 && (b->word_bytes == 8 || b->word_bytes == 2));
        max_hyp = std::max(b->max_hyp, b->S);
    } else {
        SF_CHECK_ARG(b->hyp_ids && b->hyp_off && b->max_hyp >= 0);
    }
    const int lim_hyp = sf_bleu_max_hyp(), lim_ref = sf_bleu_max_ref();
    if (b->n_dict > sf_bleu_max_dict() || max_hyp > lim_hyp || b->max_ref > lim_ref || b->n_refs > sf_bleu_max_refs())
        return SF_ERR_UNSUPPORTED;
    SF_LAUNCH(sf::bleu_counts_kernel, dim3(b->n_hyps), dim3(sf::WAVE), 0, (hipStream_t)stream, *b, lim_hyp, lim_ref, err);
    return sf::launch_status();
}
