// Corpus BLEU counted on the device (reference: tasks/R2R/eval_speaker.py:11-122, tasks/R2R/bleu.py:15-72 and the
// multi-bleu script bleu.py pipes its files through; speaker_follower_amd/speaker_evaluation.py restates them and
// bleu_count_rows there is the specification of this kernel).  Per hypothesis ten integers: clipped n-gram matches and
// n-gram totals for n = 1..4, the hypothesis length, the length of the closest reference.  Integers only: the one
// place floating point happens is speaker_evaluation.bleu_from_counts, on the host, over the ten sums.
//
// Words are ids of an evaluation-private dictionary of at most 2^16 entries, so an n-gram IS the packing of its up to
// four 16-bit ids into one 64-bit key: one compare per pair of n-grams, no hashing, nothing can collide.  n-grams of
// different orders are never compared with each other (each order has its own mask and its own counters).
#include "sf_sentences.h"

#include <atomic>

namespace sf {
namespace {

std::atomic<int> g_bleu_max_dict{SF_BLEU_MAX_DICT};
std::atomic<int> g_bleu_max_hyp{SF_BLEU_MAX_HYP};
std::atomic<int> g_bleu_max_ref{SF_BLEU_MAX_REF};
std::atomic<int> g_bleu_max_refs{SF_BLEU_MAX_REFS};

// One wavefront (= one workgroup) per hypothesis; lane l owns the hypothesis start positions l, l + 64, ...
// The staging into LDS is sf_sentences.h's, shared with caption_scores_kernel.
__global__ __launch_bounds__(WAVE) void bleu_counts_kernel(sf_bleu_batch p, int lim_hyp, int lim_ref,
                                                           int32_t* __restrict__ err) {
    __shared__ uint16_t hyp[SF_BLEU_MAX_HYP + PAD_WORDS];
    __shared__ uint16_t ref[SF_BLEU_MAX_REFS][SF_BLEU_MAX_REF + PAD_WORDS];
    const int lane = threadIdx.x, R = p.n_refs;
    int rl[SF_BLEU_MAX_REFS], H, slot;
    if (!stage_sentences(p, lim_hyp, lim_ref, hyp, ref, rl, H, slot, err)) return;
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
