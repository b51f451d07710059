// `sample` feedback of the speaker (speaker.py:170-174: probs = softmax(logit); D.Categorical(probs).sample()).
// The reference draws from torch's stateful generator, whose stream cannot be reproduced; the draw here is
// counter-based -- a pure function of (seed, stream = site + word step, GLOBAL row id) like the dropout masks and
// the follower's sampler (sf_glue.h) -- so it does not depend on how a batch is sharded, and it is the SAME
// two-level inverse-CDF draw in the per-step glue kernel (sf_pointwise.hip) and in the persistent word loop
// (sf_persist.hip), where the vocabulary is spread over 32 workgroups.  For a vocabulary of V columns:
//   ns = ceil(V / 32) slots;  slot s = columns [32 s, min(32 s + 32, V));  m_s = max, z_s = sum exp(l - m_s) over them
//   level 1 (uniform u1): the first slot IN SLOT ORDER with positive weight  z_s exp(m_s - M)  whose inclusive prefix
//                         of those weights exceeds  u1 * Z  (Z = their sum over all ns slots)
//   level 2 (uniform u2): inside that slot, the first column with positive weight whose inclusive prefix of
//                         exp(l - m_s) exceeds  u2 * z_s
// P(column c of slot s) = P(s) P(c | s) = softmax(l)_c.  Fallbacks when a threshold rounds up to the total: the slot
// of the arg max; the last valid column of the slot, min(32 s + 31, V - 1).  A slot whose columns are all -inf has
// weight 0 (wexp) and is never chosen.  oracle/rng.py mirrors the draw in float64, for any V.
// V <= 1024 (ns <= 32): one wave holds every slot at once, lanes 2 s and 2 s + 1 slot s (speaker_sample_row), and the
// persistent loop one slot per workgroup.  1024 < V <= 4096: the per-step glue alone (speaker_glue_wide_sample_kernel),
// in PANELS of 1024 columns = 32 slots: panel p holds slots 32 p .. 32 p + 31 in the same lane order, the panels are
// walked in ascending order and level 1's prefix is carried from one panel into the next -- slot order throughout.
#pragma once
#include "sf_common.h"

namespace sf {

__device__ __forceinline__ float wexp(float m, float mm) { return m == -INFINITY ? 0.f : expf(m - mm); }

__device__ __forceinline__ void sample_uniforms(uint32_t seed, uint32_t stream, uint32_t row, float* u1, float* u2) {
    const uint32_t key = dropout_row_key(seed, stream, row);
    *u1 = (float)(fmix32(key) >> 8) * (1.0f / 16777216.0f);                    // = the follower's uniform (sf_glue.h)
    *u2 = (float)(fmix32(key + 0x9E3779B9u) >> 8) * (1.0f / 16777216.0f);     // = dropout hash of column 1
}

}  // namespace sf
