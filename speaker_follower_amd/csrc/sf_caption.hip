// The parts of ROUGE-L and CIDEr-D counted on the device, next to corpus BLEU (sf_bleu.hip; the definitions are
// DESIGN.md section 2's, speaker_follower_amd/speaker_evaluation.py restates them and caption_parts_rows there is the
// specification of this kernel).  Per hypothesis: its length, the LCS length against every reference of its path
// (integers), and for n = 1..4 the squared norm of its tf-idf vector and its clipped product with every reference's
// vector (sums of non-negative float64 products).  No log, exp or sqrt here: the idf of every reference n-gram comes
// in a sorted table per order, and speaker_evaluation.caption_scores_of forms the two scores on the host.
//
// The hypothesis and its references are staged by sf_sentences.h exactly as for BLEU, and an n-gram is the same 64-bit
// key; the four orders have tables of their own because the 2-gram (x, 0) and the 4-gram (x, 0, 0, 0) pack alike.
#include "sf_sentences.h"

namespace sf {
namespace {

// every float64 product is rounded on its own, as the host's are: the sums differ from the host's by their order alone
#pragma clang fp contract(off)

constexpr int LCS_COLS = SF_BLEU_MAX_REF / WAVE;                // reference columns per lane, blocked: 8
static_assert(LCS_COLS * WAVE == SF_BLEU_MAX_REF, "a lane owns a whole number of reference columns");

// The length of the longest common subsequence of hyp[0..H) and ref[0..L): the full dynamic program, one row per
// hypothesis word.  cur[j] = max(cur[j-1], match(i, j) ? prev[j-1] + 1 : prev[j]) is a prefix maximum of
// t[j] = match ? prev[j-1] + 1 : prev[j]: lane l holds the columns 8 l .. 8 l + 7 of the row in registers, takes the
// prefix maximum of its own eight, and an exclusive maximum scan over the lanes supplies what lies to their left.  A
// column at or behind L matches nothing and only carries the maximum on, so the last column of the last lane ends up
// with the answer whatever L is.  H and L are uniform over the wave; integers only.
__device__ __forceinline__ int lcs_length(const uint16_t* hyp, int H, const uint16_t* ref, int L, int lane) {
    int word[LCS_COLS], prev[LCS_COLS];
#pragma unroll
    for (int c = 0; c < LCS_COLS; ++c) {
        const int col = lane * LCS_COLS + c;
        word[c] = col < L ? (int)ref[col] : 0x10000;            // (no 16-bit id: never a match)
        prev[c] = 0;
    }
    for (int i = 0; i < H; ++i) {
        const int hw = hyp[i];                                  // a broadcast
        int diag = __shfl_up(prev[LCS_COLS - 1], 1, WAVE);      // prev[j-1] of this lane's first column
        if (lane == 0) diag = 0;
        int run = 0;
#pragma unroll
        for (int c = 0; c < LCS_COLS; ++c) {
            const int t = word[c] == hw ? diag + 1 : prev[c];
            diag = prev[c];
            run = max(run, t);
            prev[c] = run;
        }
        int upto = run;                                         // inclusive maximum over the lanes 0 .. lane
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int below = __shfl_up(upto, off, WAVE);
            if (lane >= off) upto = max(upto, below);
        }
        int left = __shfl_up(upto, 1, WAVE);
        if (lane == 0) left = 0;
#pragma unroll
        for (int c = 0; c < LCS_COLS; ++c) prev[c] = max(prev[c], left);
    }
    return __shfl(prev[LCS_COLS - 1], WAVE - 1, WAVE);
}

// The idf of `key` in the sorted table keys[0..n): a binary search, `miss` where the table does not hold it.
__device__ __forceinline__ double idf_of(const uint64_t* __restrict__ keys, const double* __restrict__ idf, int n,
                                         uint64_t key, double miss) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && keys[lo] == key ? idf[lo] : miss;
}

// One wavefront (= one workgroup) per hypothesis; lane l owns the hypothesis start positions l, l + 64, ...
__global__ __launch_bounds__(WAVE) void caption_scores_kernel(sf_caption_batch p, int lim_hyp, int lim_ref,
                                                              int32_t* __restrict__ err) {
    __shared__ uint16_t hyp[SF_BLEU_MAX_HYP + PAD_WORDS];
    __shared__ uint16_t ref[SF_BLEU_MAX_REFS][SF_BLEU_MAX_REF + PAD_WORDS];
    const int lane = threadIdx.x, R = p.n_refs;
    int rl[SF_BLEU_MAX_REFS], H, slot;
    if (!stage_sentences(p, lim_hyp, lim_ref, hyp, ref, rl, H, slot, err)) return;

    int lcs[SF_BLEU_MAX_REFS];
#pragma unroll
    for (int r = 0; r < SF_BLEU_MAX_REFS; ++r) lcs[r] = r < R ? lcs_length(hyp, H, ref[r], rl[r], lane) : 0;

    const int first_key[4] = {0, p.n_keys1, p.n_keys1 + p.n_keys2, p.n_keys1 + p.n_keys2 + p.n_keys3};
    const int n_keys[4] = {p.n_keys1, p.n_keys2, p.n_keys3, p.n_keys4};
    double hnorm2[4] = {0, 0, 0, 0}, dot[SF_BLEU_MAX_REFS][4] = {};
    for (int i0 = 0; i0 < H; i0 += WAVE) {
        const int i = i0 + lane;
        const bool mine = i < H;
        const uint64_t ki = mine ? key_at(hyp, i) : 0;
        int in_hyp[4] = {0, 0, 0, 0}, before[4] = {0, 0, 0, 0}, in_ref[SF_BLEU_MAX_REFS][4] = {};
        count_matches(hyp, H, ki, i, in_hyp, before);
#pragma unroll
        for (int r = 0; r < SF_BLEU_MAX_REFS; ++r) {
            if (r < R) {
                int unused[4] = {0, 0, 0, 0};
                count_matches(ref[r], rl[r], ki, 0, in_ref[r], unused);
            }
        }
        // a DISTINCT n-gram counts once: at its first start position in the hypothesis
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (mine && i + n < H && !before[n]) {
                const uint64_t mask = n == 3 ? ~0ull : ((1ull << (16 * (n + 1))) - 1);
                const double idf = idf_of(p.keys + first_key[n], p.idf + first_key[n], n_keys[n], ki & mask, p.idf_miss);
                const double vh = (double)in_hyp[n] * idf;
                hnorm2[n] += vh * vh;
#pragma unroll
                for (int r = 0; r < SF_BLEU_MAX_REFS; ++r) {
                    const double vr = (double)in_ref[r][n] * idf;   // (0 behind the last reference)
                    dot[r][n] += fmin(vh, vr) * vr;
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) hnorm2[n] += __shfl_xor(hnorm2[n], off, WAVE);
#pragma unroll
        for (int r = 0; r < SF_BLEU_MAX_REFS; ++r)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) dot[r][n] += __shfl_xor(dot[r][n], off, WAVE);
    }
    // every lane holds every sum: lane l stores the l-th value of each output row (plain stores)
    int my_lcs = 0;
    double my_norm = 0, my_dot = 0;
#pragma unroll
    for (int r = 0; r < SF_BLEU_MAX_REFS; ++r) {
        if (lane == r) my_lcs = lcs[r];
        if (lane == r) my_norm = hnorm2[r];                     // (four orders, four references at most: one index)
#pragma unroll
        for (int n = 0; n < 4; ++n)
            if (lane == r * 4 + n) my_dot = dot[r][n];
    }
    if (lane == 0) p.hyp_len[slot] = H;
    if (lane < R) p.lcs[(int64_t)slot * R + lane] = my_lcs;
    if (lane < 4) p.hnorm2[(int64_t)slot * 4 + lane] = my_norm;
    if (lane < R * 4) p.dot[(int64_t)slot * R * 4 + lane] = my_dot;
}

}  // namespace
}  // namespace sf

extern "C" int sf_caption_scores(const sf_caption_batch* b, int32_t* err, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(b && err && b->n_hyps >= 1 && b->n_slots >= 1 && b->n_refs >= 1 && b->n_dict >= 1 && b->max_ref >= 0 &&
                 b->ref_ids && b->ref_off && b->slot && b->keys && b->idf && b->hyp_len && b->lcs && b->dot && b->hnorm2 &&
                 b->n_keys1 >= 0 && b->n_keys2 >= 0 && b->n_keys3 >= 0 && b->n_keys4 >= 0 &&
                 (int64_t)b->n_keys1 + b->n_keys2 + b->n_keys3 + b->n_keys4 <= INT32_MAX);
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
    SF_LAUNCH(sf::caption_scores_kernel, dim3(b->n_hyps), dim3(sf::WAVE), 0, (hipStream_t)stream, *b, lim_hyp, lim_ref,
              err);
    return sf::launch_status();
}
