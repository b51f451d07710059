// A hypothesis and the references of its path staged in LDS as 16-bit dictionary ids: what bleu_counts_kernel
// (sf_bleu.hip) and caption_scores_kernel (sf_caption.hip) both start from, written once.  `Batch` is sf_bleu_batch or
// sf_caption_batch: the two name their inputs alike (n_hyps .. slot), and both forms of hypotheses -- packed ids, a
// decode's [S, n_hyps] word matrix through the vocabulary -> dictionary remap -- are read here.
//
// An n-gram IS the packing of its up to four 16-bit ids into one 64-bit key: key_at / count_matches.
#pragma once
#include "sf_common.h"

namespace sf {

constexpr int PAD_WORDS = 4;                    // behind every staged sentence: the rolling key reads w[j + 4]

typedef uint16_t staged_refs[SF_BLEU_MAX_REF + PAD_WORDS];

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

template <class Batch>
__device__ __forceinline__ int64_t word_at(const Batch& p, int s, int b) {
    const int64_t at = (int64_t)s * p.n_hyps + b;
    return p.word_bytes == 8 ? ((const int64_t*)p.words)[at] : (int64_t)((const int16_t*)p.words)[at];
}

// Hypothesis blockIdx.x (one wavefront = one workgroup each) into hyp[0..H), the n_refs references of its slot into
// ref[r][0..rl[r]), PAD_WORDS zeros behind each.  Returns false -- uniformly over the wave -- where there is nothing
// to score (no such hypothesis, slot -1) or something is inconsistent (err[0] raised, nothing may be written): a slot
// outside [-1, n_slots), an id outside the dictionary or the vocabulary, a length above the limits, offsets that
// decrease.  On true the block has passed a barrier: every lane sees the staged words.
template <class Batch>
__device__ __forceinline__ bool stage_sentences(const Batch& p, int lim_hyp, int lim_ref, uint16_t* hyp, staged_refs* ref,
                                                int rl[SF_BLEU_MAX_REFS], int& H_out, int& slot_out,
                                                int32_t* __restrict__ err) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= p.n_hyps) return false;
    const int slot = p.slot[b];                                 // (uniform over the wave, as every return below)
    if (slot == -1) return false;
    if (slot < -1 || slot >= p.n_slots) {
        if (lane == 0) *err = 1;
        return false;
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
        return false;
    }
    H_out = H;
    slot_out = slot;
    return true;
}

}  // namespace sf
