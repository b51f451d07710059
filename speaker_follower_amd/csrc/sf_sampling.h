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
// P(column c of slot s) = P(s) P(c | s) = softmax(l)_c.  "Positive weight" is meant in float32: a column more than
// ~104 below its slot's maximum, or -inf, has weight expf(.) = 0 and is never drawn, whatever the prefix sums say.
// The edges of the contract, the same in all three kernels and in the float64 mirror (oracle/rng.py::speaker_sample):
//   - a slot with no finite column has weight 0 (wexp: its m_s = -inf must not turn l - m_s into NaN, neither in
//     z_s nor in the slot's weight) and is never chosen; the prefix of level 1 walks over it;
//   - a row with no finite column at all stays outside the contract: nothing is promised about its word;
//   - fallbacks when a threshold rounds up to the total (each lane's float32 prefix is rounded in an order of its
//     own, so at u = 1 - 2^-24 no item may pass): level 1 takes the slot of the arg max; level 2 takes the LAST COLUMN
//     OF THE SLOT WHOSE WEIGHT IS POSITIVE -- not min(32 s + 31, V - 1), which may be a banned or underflowed word.
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
