/* sf_hip.h -- C ABI of libsf_hip.so: the speaker/follower hot path on MI355X (gfx950).
 *
 * The reference (ronghanghu/speaker_follower) has no C FFI for this path: its operator API is
 * the set of torch.nn.Module classes in tasks/R2R/model.py plus the per-step tensor glue in
 * tasks/R2R/follower.py and speaker.py.  Each entry point below replaces the arithmetic of one of
 * those functions (cited as file:line under /root/reference) and is what a binding written
 * against the reference would call -- see INTEGRATION.md for the ctypes stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless stated; fp32 row-major; leading dimensions in
 *     elements; index arrays int32 unless stated; masks uint8 (1 = masked / padded);
 *   - nothing allocates, frees or synchronises: outputs, saved activations and the scratch
 *     workspace are passed in; all work is enqueued on `stream` (a hipStream_t; NULL = default);
 *     calls are safe inside hipGraph stream capture;
 *   - return value: SF_OK or an SF_ERR_* code; no global state, thread-safe per stream as long as
 *     concurrent calls use different workspaces;
 *   - "accumulate" outputs (weight gradients, dctx) are read-modify-write: the caller zeroes them
 *     once per backward pass.  Gradient structs mirror the weight structs; a NULL member skips
 *     that gradient.
 *   - dropout is counter based: keep(seed, stream_id, global_row, col) -- see sf_dropout.
 */
#ifndef SF_HIP_H_
#define SF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_ABI_VERSION 10

enum {
    SF_OK = 0,
    SF_ERR_ARG = 1,         /* null pointer, non-positive size, misaligned leading dimension */
    SF_ERR_UNSUPPORTED = 2, /* shape outside what the kernels are built for */
    SF_ERR_LAUNCH = 3,      /* hipGetLastError() reported a launch failure */
    SF_ERR_WORKSPACE = 4    /* workspace too small (see sf_workspace_bytes) */
};

typedef void* sf_stream;

/* nn.Dropout(p) replacement (model.py:52, 370, 414, 473).  p == 0 => eval mode.  The mask for
 * element (row, col) of dropout site `stream_id` is a pure function of (seed, stream_id,
 * row0 + row, col); oracle/rng.py mirrors it bit for bit. */
typedef struct sf_dropout {
    float p;
    uint32_t seed;
    int32_t row0; /* global id of local row 0 (data-parallel shards pass their offset) */
    /* Device-side site offset (ABI 8, optional: NULL = none).  A kernel forms its mask for site
     * `stream_id + site_mul * *site_dev`: the stream ids the host passes are then RELATIVE to a counter that lives in
     * device memory, and a hipGraph that captured a training iteration draws fresh masks on every replay once
     * sf_site_advance (captured at the end of the iteration) has moved the counter -- kernel arguments are frozen in a
     * graph, device memory is not.  Entry points that number their sites 2 * step_id + k internally (the decoder
     * steps) scale the offset by 2 themselves; site_mul (0 = 1) scales it for entry points that take a raw stream
     * id, so that host and device numbering agree: a replay draws exactly the masks of the eager iteration whose
     * host-side site counter equals the device word. */
    const uint32_t* site_dev;
    uint32_t site_mul;
} sf_dropout;
/* *word += by, on the stream (one thread): advances a device-side site counter (sf_dropout.site_dev,
 * sf_sample.stream_dev, sf_follower_glue.sample_site_dev). */
int sf_site_advance(uint32_t* word, uint32_t by, sf_stream stream);
/* dst[0..3] = a, b, c, d on the stream (values travel as kernel arguments: no host buffer to keep alive).  How the host
 * hands a replayed training graph its per-replay inputs -- site counter and optimizer step counters -- in ONE tiny
 * launch in front of the graph launch (runtime.TrainingGraph). */
int sf_store_u32x4(uint32_t* dst, uint32_t a, uint32_t b, uint32_t c, uint32_t d, sf_stream stream);

/* Panorama rows of a batch: either the dense [B,V,F] tensor the reference's
 * Seq2SeqAgent._feature_variables builds (follower.py:291-298, env.py:330-332, 771-773) or the
 * HBM-resident feature table addressed by index (replaces env.py:380-383 dict lookup + np.stack +
 * H2D copy): row v of sample b = table[vp[b], v, :] || loc_table[view[b], v, :]. */
typedef struct sf_pano {
    const float* dense;     /* [B,V,IMG+LOC] or NULL */
    const float* table;     /* [n_viewpoints, V, IMG] */
    const float* loc_table; /* [V, V, LOC]  (env.py:78-101) */
    const int32_t* vp;      /* [B]; < 0 => all-zero panorama (speaker.py:93-95 padded step) */
    const int32_t* view;    /* [B]; clamped into [0, V) */
    int32_t V, IMG, LOC;
} sf_pano;

/* Candidate-action rows: dense all_u_t [B,A,F] (follower.py:300-320) or by index
 * (env.py:60-75): row a>0 = table[vp[b], cand_view[b,a], :] || sin/cos(rel_heading, rel_elevation)
 * each repeated LOC/4 times; row 0 (stop) and rows >= a_num[b] are zero. */
typedef struct sf_cands {
    const float* dense;       /* [B,A,IMG+LOC] or NULL */
    const float* table;
    const int32_t* vp;        /* [B] */
    const int32_t* cand_view; /* [B,A] */
    const float* cand_sincos; /* [B,A,4]: sin h, cos h, sin e, cos e */
    const int32_t* a_num;     /* [B] */
    int32_t A, V, IMG, LOC;
} sf_cands;

/* ---- weights (pointer sets keyed like the reference state_dicts) -------------------------- */
/* Members ending in _t are OPTIONAL transposed copies (sf_transpose) of the weight of the same
 * name: with them every product on the path, forward and backward, is K-contiguous (288 GB of HBM
 * make a second layout of the hot weights free); NULL falls back to the slower in-place form.
 * Gradient structs mirror the weight structs member for member (the _t slots are ignored). */
typedef struct sf_lstm_w { /* nn.LSTMCell / nn.LSTM layer 0: weight_ih [4H,I], weight_hh [4H,H] */
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    const float *w_ih_t, *w_hh_t; /* [I,4H], [H,4H] */
} sf_lstm_w;
typedef struct sf_lstm_g { float *w_ih, *w_hh, *b_ih, *b_hh, *unused0, *unused1; } sf_lstm_g;

typedef struct sf_visual_w { /* VisualSoftDotAttention model.py:303-308 */
    const float *w_h, *b_h; /* linear_in_h [D,H],[D] */
    const float *w_v, *b_v; /* linear_in_v [D,F],[D]; b_v cannot change the output (softmax shift) */
    const float *w_v_t;     /* [F,D] */
    const float *w_h_t;     /* [H,D] */
} sf_visual_w;
typedef struct sf_visual_g { float *w_h, *b_h, *w_v, *b_v, *unused0, *unused1; } sf_visual_g;

typedef struct sf_softdot_w { /* SoftDotAttention model.py:114-120 */
    const float *w_in;  /* linear_in  [H,H]  (no bias) */
    const float *w_out; /* linear_out [H,2H] (no bias) */
    const float *w_in_t, *w_out_t; /* [H,H], [2H,H] */
} sf_softdot_w;
typedef struct sf_softdot_g { float *w_in, *w_out, *unused0, *unused1; } sf_softdot_g;

typedef struct sf_scoring_w { /* EltwiseProdScoring model.py:335-340 */
    const float *w_h, *b_h;     /* linear_in_h [D,H],[D] */
    const float *w_a, *b_a;     /* linear_in_a [D,F],[D] */
    const float *w_out, *b_out; /* linear_out  [1,D],[1] */
    const float *w_a_t;         /* [F,D] */
    const float *w_h_t;         /* [H,D] */
} sf_scoring_w;
typedef struct sf_scoring_g { float *w_h, *b_h, *w_a, *b_a, *w_out, *b_out, *unused0, *unused1; } sf_scoring_g;

/* Consecutive Linears folded into one matrix each (built by sf_decoder_fold_build once per weight
 * version): the visual query q = W_v^T (W_h h + b_h) is q = M_v h + c_v, and the scoring vector /
 * constant r = W_a^T (w_out * (W_h h~ + b_h)), c = wt.b_a + b_out are [r | c] = M_a h~ + c_a.
 * sf_projected_build forms the projected feature tables from them; no decode step reads them. */
typedef struct sf_decoder_fold {
    const float* m_v; /* [F,H]   = W_v^T W_h */
    const float* c_v; /* [F]     = W_v^T b_h */
    const float* m_a; /* [F+4,H]: rows < F = W_a^T diag(w_out) W_h; row F = W_h^T (w_out*b_a); rest 0 */
    const float* c_a; /* [F+4]:   [< F] = W_a^T (w_out*b_h); [F] = (w_out*b_h).b_a + b_out; rest 0 */
} sf_decoder_fold;
typedef struct sf_decoder_w { /* AttnDecoderLSTM model.py:361-375 */
    sf_lstm_w lstm;       /* LSTMCell(2F -> H) */
    sf_visual_w visual;
    sf_softdot_w text;
    sf_scoring_w action;
} sf_decoder_w;
typedef struct sf_decoder_g { sf_lstm_g lstm; sf_visual_g visual; sf_softdot_g text; sf_scoring_g action; } sf_decoder_g;

/* ---- saved activations of one AttnDecoderLSTM step (all written by fwd, read by bwd) ------- */
typedef struct sf_decoder_tape {
    float* t_v;     /* [B,D]   linear_in_h(h0) */
    float* q;       /* [B,F]   t_v folded through linear_in_v */
    float* alpha_v; /* [B,V] */
    float* xin;     /* [B,2F]  dropout(cat(u_prev, feature)) -- LSTM input */
    float* gates;   /* [B,4H]  activated gates i,f,g,o */
    float* c1;      /* [B,H] */
    float* h1;      /* [B,H]   (un-dropped, returned) */
    float* cat2;    /* [B,2H]  cat(weighted_ctx, dropout(h1)) -- linear_out input */
    float* t_text;  /* [B,H]   linear_in(dropout(h1)) */
    float* alpha;   /* [B,L] */
    float* h_tilde; /* [B,H] */
    float* t_a;     /* [B,D]   linear_in_h(h_tilde) (before the w_out product) */
    float* wt;      /* [B,D]   t_a * linear_out.weight */
    float* r;       /* [B,F]   wt folded through linear_in_a */
    float* logit;   /* [B,A]   raw logits (unmasked) */
} sf_decoder_tape;

/* Scratch any call may need (split-K partial slabs etc.); a constant, independent of batch. */
/* Size of the scratch buffer every composite entry point takes.  The caller ZERO-FILLS it once
 * after allocation (its last 4 KB hold self-maintaining ticket counters of multi-workgroup
 * kernels); after that the library owns its contents.  One workspace per concurrently used stream. */
size_t sf_workspace_bytes(void);
/* Recommended size of the scratch buffer handed to the WEIGHT-GRADIENT entry points (sf_attn_decoder_wgrad): with this
 * much they form the decoder's small weight gradients in three grouped launches (transposed operands + K-split slabs of
 * all of them at once); with sf_workspace_bytes() they fall back to one product at a time.  No zero-fill needed; a
 * buffer of its own -- not a bigger workspace for every call: the decode steps run 2 % slower over a 256 MB workspace. */
size_t sf_wgrad_workspace_bytes(void);
int sf_abi_version(void);
/* Hash (16 hex digits) of the sources, headers and compiler flags this library was built from
 * (speaker_follower_amd/build.py: build_id()).  The Python binding compares it with the sources on disk at import
 * and refuses a stale library. */
const char* sf_build_id(void);
const char* sf_status_string(int status);
/* hipGetErrorString of the HIP error behind the calling thread's last SF_ERR_LAUNCH */
const char* sf_last_error_string(void);

/* ---- nn.Linear (model.py:64, 99, 117-119, 306-307, 338-340, 419, 485) ------------------------
 * y[M,N] = act(x[M,K] w[N,K]^T + b);  act: 0 none, 1 tanh.  K % 4 == 0, ldx % 4 == 0.
 * Outside the operands the call reads and writes NOTHING: of x only rows < M and columns < K (the K..ldx-1 padding of
 * a row and whatever lies behind row M-1 belong to someone else -- the engines pass views into wider rows -- and may
 * hold NaN), of y only rows < M and columns < N are written (columns N..ldy-1 and the rows behind keep their
 * contents).  tests/test_gpu_gemm_dispatch.py holds every kernel of the dispatch to this. */
int sf_linear_fwd(const float* x, int ldx, const float* w, const float* b, int M, int N, int K,
                  int act, float* y, int ldy, void* ws, size_t ws_bytes, sf_stream stream);
/* The product alone, as split-K partial slabs (what the LSTM cell consumes: its pointwise kernel
 * adds the slabs, the biases and applies the gates -- model.py:393): x [M,K1] w [N,K1]^T +
 * h [M,K2] u [N,K2]^T (h, u may be NULL) -> *ksplit slabs [ksplit][M][N] at the START of the
 * workspace (ksplit >= 1 is returned; the caller sums them).  This is the entry point bench.py
 * times for its roofline object: exactly one launch of the gate-product kernel. */
int sf_linear_slabs_fwd(const float* x, int ldx, const float* w, int K1, const float* h, int ldh,
                        const float* u, int K2, int M, int N, int* ksplit, void* ws, size_t ws_bytes,
                        sf_stream stream);
/* dy is the gradient wrt the activation output; y is the saved output (needed for act = tanh).
 * dx [M,K] overwritten (accumulate_dx = 0) or added to; dw [N,K], db [N] accumulated.
 * As for sf_linear_fwd, nothing outside the operands is read or written: x [M,K], y and dy [M,N] are read at rows < M
 * and columns < K resp. N only (padding columns up to ldx / ldy / lddy and rows behind M-1 may hold NaN); of dx only
 * rows < M, columns < K are written (columns K..lddx-1 and the rows behind keep their contents). */
int sf_linear_bwd(const float* x, int ldx, const float* w, const float* y, int ldy,
                  const float* dy, int lddy, int M, int N, int K, int act, float* dx, int lddx,
                  int accumulate_dx, float* dw, float* db, void* ws, size_t ws_bytes,
                  sf_stream stream);

/* ---- nn.LSTMCell (model.py:371/393, 417-418/434, 483/515), gate order i,f,g,o -----------------
 * x [B,I] (I % 4 == 0).  Writes h1,c1 [B,H] and the activated gates [B,4H] for the backward.
 * If h1_drop != NULL also writes dropout(h1) there (row stride ld_h1_drop; site `drop_stream`). */
int sf_lstm_cell_fwd(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx,
                     const float* h0, const float* c0, float* h1, float* c1, float* gates,
                     float* h1_drop, int ld_h1_drop, const sf_dropout* drop, uint32_t drop_stream,
                     void* ws, size_t ws_bytes, sf_stream stream);
/* dh1,dc1 [B,H] in (NULL = zero); dx [B,I] (lddx), dh0, dc0 out (overwritten); weight grads
 * accumulated. */
int sf_lstm_cell_bwd(const sf_lstm_w* w, const sf_lstm_g* g, int B, int I, int H, const float* x,
                     int ldx, const float* h0, const float* c0, const float* c1,
                     const float* gates, const float* dh1, const float* dc1, float* dx, int lddx,
                     float* dh0, float* dc0, void* ws, size_t ws_bytes, sf_stream stream);

/* ---- VisualSoftDotAttention.forward (model.py:310-326) ---------------------------------------
 * out[b, :F] (row stride ldo) = sum_v alpha[b,v] X[b,v,:], alpha = softmax_v((W_v x_v + b_v).t),
 * t = W_h h + b_h.  Implemented as softmax_v(x_v . q), q = W_v^T t (b_v.t is a per-row constant and
 * cancels in the softmax), so X is read once and the [B*V,F]x[F,D] product disappears.
 * Optional dropout on `out` (site drop_stream, column offset drop_col0 -- the fused decoder writes
 * straight into the LSTM input buffer).  t_v [B,D] and q [B,F] are saved for the backward. */
int sf_visual_attention_fwd(const sf_visual_w* w, const sf_pano* X, int B, int H, int D,
                            const float* h, float* out, int ldo, float* alpha, float* t_v,
                            float* q, const sf_dropout* drop, uint32_t drop_stream,
                            int drop_col0, void* ws, size_t ws_bytes, sf_stream stream);
/* The same function with every intermediate rounded ONCE (round 5, csrc/sf_precise.hip): t = W_h h + b_h and
 * q = W_v^T t are formed on the float64 matrix cores (v_mfma_f64_16x16x4_f64) and kept in float64, the scores x_v . q
 * are accumulated in float64, the softmax sees them relative to their maximum.  What the speaker's path encoder runs
 * (sf_speaker_encoder_fwd): with the reference's "peaky" weights its scores reach +-80, where an fp32 evaluation of
 * the chain -- the reference's own included -- leaves 2e-6 .. 9e-6 of roundoff per stage in the softmax weights and
 * 1e-4 .. 3e-4 in the word logits behind the 7-step context.  t_v / q receive fp32 copies (the backward's tapes).
 * SF_ERR_UNSUPPORTED outside V in (18, 36], B <= 256, no transposed W_v copy: call sf_visual_attention_fwd. */
int sf_visual_attention_fwd_f64(const sf_visual_w* w, const sf_pano* X, int B, int H, int D,
                                const float* h, float* out, int ldo, float* alpha, float* t_v,
                                float* q, const sf_dropout* drop, uint32_t drop_stream,
                                int drop_col0, void* ws, size_t ws_bytes, sf_stream stream);
/* y = x W^T + b with float64 accumulation on the float64 matrix cores: x [M,K] fp32 (row stride ldx), W [N,K] fp32
 * (row stride ldw), b [N] or NULL; y64 [M,N] float64 and / or y32 [M,N] fp32 (either may be NULL).  K, ldx, ldw
 * multiples of 4. */
int sf_linear_f64(const float* x, int ldx, const float* w, int ldw, const float* b, int M, int N, int K,
                  double* y64, float* y32, sf_stream stream);
/* dout [B,F] (row stride lddo) is the gradient wrt the (dropped) output; dh [B,H] is ADDED to. */
int sf_visual_attention_bwd(const sf_visual_w* w, const sf_visual_g* g, const sf_pano* X, int B,
                            int H, int D, const float* h, const float* alpha, const float* t_v,
                            const float* dout, int lddo, const sf_dropout* drop,
                            uint32_t drop_stream, int drop_col0, float* dh, void* ws,
                            size_t ws_bytes, sf_stream stream);

/* ---- SoftDotAttention.forward (model.py:122-143) ---------------------------------------------
 * h [B,H] (row stride ldh); ctx [B,L,H]; mask [B,L] uint8 or NULL.  Writes alpha [B,L], h_tilde
 * [B,H] and the saved cat2 = [weighted_ctx ; h] [B,2H], t_text = linear_in(h) [B,H].
 * ctx_row (int32 [B] or NULL): sample b attends over ctx[ctx_row[b]] / mask[ctx_row[b]] -- the
 * search procedures' `ctx[beam_indices]` (follower.py:580, 790; speaker.py:252) without the copy.
 * Forward only: the backward entry points expect ctx_row == NULL in the forward pass. */
int sf_soft_dot_attention_fwd(const sf_softdot_w* w, int B, int L, int H, const float* h, int ldh,
                              const float* ctx, const uint8_t* mask, const int32_t* ctx_row,
                              float* h_tilde, float* alpha, float* cat2, float* t_text, void* ws,
                              size_t ws_bytes, sf_stream stream);
/* dh_tilde [B,H] in; dh [B,H] (row stride lddh) overwritten; dctx [B,L,H] ADDED to (NULL = skip). */
int sf_soft_dot_attention_bwd(const sf_softdot_w* w, const sf_softdot_g* g, int B, int L, int H,
                              const float* ctx, const float* alpha, const float* cat2,
                              const float* t_text, const float* h_tilde, const float* dh_tilde,
                              float* dh, int lddh, float* dctx, void* ws, size_t ws_bytes,
                              sf_stream stream);

/* ---- ContextOnlySoftDotAttention.forward behind its linear_in (model.py:166-177; SpeakerDecoderLSTM with
 * use_input_att_feed, model.py:500-503): attn = softmax_l(ctx[b,l,:] . t[b,:]) with mask[b,l] != 0 -> -inf,
 * wc[b,:] = sum_l attn[b,l] ctx[b,l,:].  ctx [B,L,H], mask [B,L] uint8 or NULL, t [B,H] (row stride ldt) = linear_in(h),
 * alpha [B,L], wc [B,H] (row stride ldwc). */
int sf_text_attention_fwd(const float* ctx, const uint8_t* mask, int B, int L, int H, const float* t, int ldt,
                          float* alpha, float* wc, int ldwc, sf_stream stream);
/* dwc [B,H] in; dt [B,H] out (overwritten); dctx [B,L,H] accumulated (NULL: not formed). */
int sf_text_attention_bwd(const float* ctx, int B, int L, int H, const float* dwc, int lddwc, const float* t, int ldt,
                          const float* alpha, float* dt, int lddt, float* dctx, sf_stream stream);

/* ---- EltwiseProdScoring.forward (model.py:342-352) -------------------------------------------
 * logit[b,a] = w_out . (t_a[b] * (W_a u[b,a] + b_a)) + b_out,  t_a = W_h h + b_h; implemented as
 * u[b,a] . r[b] + wt[b] . b_a + b_out with wt = w_out * t_a, r = W_a^T wt.  Saves t_a, wt [B,D], r. */
int sf_eltwise_prod_scoring_fwd(const sf_scoring_w* w, const sf_cands* U, int B, int H, int D,
                                const float* h, float* logit, float* t_a, float* wt, float* r,
                                void* ws, size_t ws_bytes, sf_stream stream);
/* dlogit [B,A] in; dh [B,H] overwritten. */
int sf_eltwise_prod_scoring_bwd(const sf_scoring_w* w, const sf_scoring_g* g, const sf_cands* U,
                                int B, int H, int D, const float* h, const float* t_a,
                                const float* wt, const float* dlogit, float* dh, void* ws,
                                size_t ws_bytes, sf_stream stream);

/* ---- follower per-step glue (follower.py:476-505) ---------------------------------------------
 * Masks logits of invalid candidates to -inf in place (valid = a < a_num[b], or is_valid[b,a] != 0
 * when is_valid is given), computes the cross-entropy term against target[b] (int64, -1 = ignore;
 * rows with ended[b] != 0 are forced to -1), chooses the next action (feedback 0 = teacher:
 * max(target,0); 1 = argmax, first maximum; 2 = sample from softmax with a counter-based uniform),
 * writes this step's score[b] = log p(a_t) (the caller sums steps: follower.py:504-505), writes
 * u_next[b,:] = U[b, a_t, :] (optionally through the NEXT step's input dropout, so that it can land
 * directly in that step's LSTM input buffer), updates ended[b] |= (a_t == 0).  ce_term[b] / live[b]
 * receive the row's CE term and 0/1 liveness; target_used the effective targets for the backward.
 * The sample (feedback 2): one uniform u per row, the top 24 bits of the hash of (sample_seed, sample_stream +
 * *sample_site_dev, row0 + b), column 0 (oracle/rng.py: sample_uniforms, follower_sample).  With e = expf(l - max) over the
 * valid candidates, the action is the first candidate with e > 0 whose inclusive float32 prefix sum exceeds u * sum e;
 * if there is none (u * sum within an ulp of the total) it is the highest candidate with e > 0.  A candidate whose float32
 * weight underflowed to 0 is never drawn, at u = 1 - 2^-24 either. */
typedef struct sf_follower_glue {
    const float* is_valid;    /* [B,A] or NULL */
    const int64_t* target;    /* [B] */
    int32_t feedback;
    uint8_t* ended;           /* [B] in/out */
    int64_t* a_t;             /* [B] out */
    int64_t* target_used;     /* [B] out */
    float* score;             /* [B] out */
    float* u_next;            /* [B, ld_u_next] out, or NULL */
    int32_t ld_u_next;
    const sf_dropout* u_drop; /* NULL = no dropout on u_next */
    uint32_t u_drop_stream;
    float* ce_term;           /* [B] out */
    float* live;              /* [B] out */
    uint32_t sample_seed, sample_stream; /* feedback 2 only */
    int32_t row0;                        /* global id of row 0 (sampling stream) */
    const uint32_t* sample_site_dev;     /* ABI 8, optional: device word added to sample_stream (sf_dropout.site_dev) */
    /* optional (scoring + glue launch only): env.step + env.observe + teacher of a device-resident
     * environment right behind the action choice, instead of a separate sf_nav_step launch */
    const struct sf_nav_io* nav;
} sf_follower_glue;
/* SF_ERR_UNSUPPORTED for A > 64 and, with index-form candidates (U->dense == NULL), unless IMG % 4 == 0 && LOC % 16 == 0
 * (the row layout of u_next, see the batched feature gathers below); nothing is launched, nothing written. */
int sf_follower_glue_fwd(const sf_cands* U, int B, float* logit, const sf_follower_glue* glue,
                         sf_stream stream);
/* dlogit[b,a] = gscale[0] * (softmax(logit)[b,a] - [a == target_used[b]]) for live rows, else 0
 * (gscale = dloss / live count: a device scalar, so no host sync is needed). */
int sf_follower_glue_bwd(int B, int A, const float* logit, const int64_t* target_used,
                         const float* gscale, float* dlogit, sf_stream stream);

/* ---- AttnDecoderLSTM.forward (model.py:377-397): one follower decode step --------------------
 * u_prev [B,F] (NULL = tape->xin[:, :F] already holds dropout(u_prev), e.g. written by the
 * previous step's glue); X panorama; U candidates; h0,c0 [B,H]; ctx [B,L,H]; ctx_mask [B,L].
 * Returns h1,c1 (tape->h1, tape->c1), alpha (tape->alpha), logit (tape->logit), alpha_v.
 * With glue != NULL the per-step glue runs fused with the scoring kernel and tape->logit holds
 * the MASKED logits (what sf_follower_glue_bwd wants); otherwise the raw logits.
 * ctx_row: see sf_soft_dot_attention_fwd (search: many states share one instruction context).
 * Dropout sites: 2*step for the LSTM input, 2*step+1 for h1 (step = `step_id`). */
int sf_attn_decoder_fwd(const sf_decoder_w* w, const sf_pano* X, const sf_cands* U, int B, int H,
                        int D, int L, const float* u_prev, const float* h0, const float* c0,
                        const float* ctx, const uint8_t* ctx_mask, const int32_t* ctx_row,
                        const sf_decoder_tape* tape, const sf_follower_glue* glue,
                        const sf_dropout* drop, uint32_t step_id, void* ws, size_t ws_bytes,
                        sf_stream stream);
/* The same step, software-pipelined across steps (what a rollout over index-form observations
 * uses).  Given h1 of step t, the visual half of step t+1 (linear_in_h, W_v^T t, visual attention:
 * model.py:389 of the NEXT call) does not depend on the text attention / scoring half of step t,
 * so the two run side by side in paired launches:
 *   head(t):  t_v, q, visual attention           -> tape->xin[:, F:2F], alpha_v
 *   tail(t):  LSTMCell, text attention, scoring (+glue) of step t; if X_next != NULL also head(t+1)
 *             from h1 of step t into tape_next.
 * A rollout is head(0), tail(0; X_1), tail(1; X_2), ..., tail(S-1; NULL); results are identical to
 * S calls of sf_attn_decoder_fwd (same kernels, same tapes: the backward entry points apply). */
int sf_attn_decoder_head_fwd(const sf_decoder_w* w, const sf_pano* X, int B, int H, int D,
                             const float* h0, const sf_decoder_tape* tape, const sf_dropout* drop,
                             uint32_t step_id, void* ws, size_t ws_bytes, sf_stream stream);
/* When the next panorama depends on this step's action (a device-resident environment: nav.py), call the
 * tail with X_next = NULL and tape_next != NULL: only the QUERY of step t+1's visual attention (t_v', q':
 * functions of h1) is formed beside the text stages; after the environment step, sf_attn_decoder_attend_fwd
 * runs the attention of step t+1 from tape->q into tape->xin[:, F:2F] / tape->alpha_v (model.py:310-326). */
int sf_attn_decoder_attend_fwd(const sf_pano* X, int B, const sf_decoder_tape* tape, const sf_dropout* drop,
                               uint32_t step_id, void* ws, size_t ws_bytes, sf_stream stream);
int sf_attn_decoder_tail_fwd(const sf_decoder_w* w, const sf_cands* U, int B, int H, int D, int L,
                             const float* u_prev, const float* h0, const float* c0,
                             const float* ctx, const uint8_t* ctx_mask, const int32_t* ctx_row,
                             const sf_decoder_tape* tape, const sf_follower_glue* glue,
                             const sf_dropout* drop, uint32_t step_id, const sf_pano* X_next,
                             const sf_decoder_tape* tape_next, void* ws, size_t ws_bytes,
                             sf_stream stream);

/* Per-step gradient tape: the "dY" operands of every weight-gradient product of one decoder step.
 * BPTT over S steps keeps them stacked [S][B][..]; sf_attn_decoder_wgrad then forms each weight
 * gradient ONCE with reduction depth S*B instead of S read-modify-write passes over 12 M weights. */
typedef struct sf_decoder_gtape {
    float* dgates;  /* [B,4H] LSTM pre-activation gate gradients */
    float* dpre;    /* [B,H]  linear_out pre-activation gradient */
    float* dt_text; /* [B,H]  gradient of linear_in(h1_drop) */
    float* dt_v;    /* [B,D]  gradient of visual linear_in_h(h0) */
    float* dq;      /* [B,F]  gradient of the folded visual query */
    float* dwt;     /* [B,D]  gradient of wt = t_a * w_out */
    float* dta;     /* [B,D]  gradient of t_a */
    float* dr;      /* [B,F]  gradient of the folded scoring vector */
    float* dc;      /* [B]    gradient of the per-row scoring constant */
    /* optional (NULL = dctx is updated by every step's text-attention backward): with both given,
     * sf_follower_episode_bwd keeps each step's d[wc ; h1_drop] and d(score) here and adds
     * dctx += sum_t (alpha_t (x) dwc_t + ds_t (x) t_text_t) ONCE after the loop, instead of a
     * read-modify-write of the [B,L,H] gradient per step */
    float* dcat2;   /* [B,2H] gradient of [weighted context ; dropout(h1)] */
    float* ds;      /* [B,L]  gradient of the text-attention scores */
    /* optional (episode backward with a side stream): the attention path's share of d h1, per step */
    float* dh1d;    /* [B,H] */
} sf_decoder_gtape;
/* Builds the sf_decoder_fold matrices from the (transposed copies of the) decoder weights:
 * m_v [F,H], c_v [F], m_a [F+4,H], c_a [F+4] are caller-allocated device buffers. */
int sf_decoder_fold_build(const sf_decoder_w* w, int H, int D, int F, float* m_v, float* c_v,
                          float* m_a, float* c_a, void* ws, size_t ws_bytes, sf_stream stream);

/* Gradients in: dlogit [B,A], dh1, dc1 [B,H] (NULL = zero).  Out: dh0, dc0 [B,H] overwritten,
 * dctx [B,L,H] ADDED to.  u_prev is detached in the reference (follower.py:502): no du_prev.
 * g != NULL: weight gradients of this step are accumulated immediately; gtape != NULL: the dY
 * operands are saved there for a later sf_attn_decoder_wgrad (pass g = NULL then). */
int sf_attn_decoder_bwd(const sf_decoder_w* w, const sf_decoder_g* g, const sf_pano* X,
                        const sf_cands* U, int B, int H, int D, int L, const float* h0,
                        const float* c0, const float* ctx, const sf_decoder_tape* tape,
                        const sf_decoder_gtape* gtape, const float* dlogit, const float* dh1,
                        const float* dc1, float* dh0, float* dc0, float* dctx,
                        const sf_dropout* drop, uint32_t step_id, void* ws, size_t ws_bytes,
                        sf_stream stream);
/* Weight gradients of M = S*B stacked rows: `tape` / `gtape` point at step 0 of stacked
 * [S][B][..] tensors, h0_all [M,H] holds every step's incoming hidden state. */
int sf_attn_decoder_wgrad(const sf_decoder_w* w, const sf_decoder_g* g, int M, int H, int D, int F,
                          const float* h0_all, const sf_decoder_tape* tape,
                          const sf_decoder_gtape* gtape, void* ws, size_t ws_bytes,
                          sf_stream stream);

/* ---- a whole follower episode in one call (follower.py:430-539 forward, :1014-1016 backward) ----
 * All per-step tensors of an index-form (or dense) episode are stacked [S][...] arrays: `X`, `U`,
 * `tape`, `glue` hold the pointers of STEP 0 and step t lives t * (per-step size) further on (sizes
 * follow from S, B, H, D, L, A and the feature dims; tape.xin has S+1 steps, glue.ended is [B]).
 * glue.u_next / ld_u_next / u_drop / u_drop_stream / sample_stream are ignored: u_next of step t
 * always goes, through the next step's input dropout, into tape.xin of step t+1.
 * fwd  = sf_attn_decoder_head_fwd(0) then S x sf_attn_decoder_tail_fwd, with no host work between.
 *        glue.nav != NULL (sf_nav_io of STEP 0 of a device-resident environment, state buffers stacked
 *        [S + 1][...]): per step sf_attn_decoder_tail_fwd with tape_next but no X_next -- the environment steps
 *        inside its scoring + glue launch -- followed by sf_attn_decoder_attend_fwd over the panorama just chosen
 *        (needs w->visual.w_v_t).
 * bwd  = per step t = S-1..0: sf_follower_glue_bwd (gscale[t]) + sf_attn_decoder_bwd (g = NULL, dY
 *        operands into the stacked gtape), ping-ponging (dh, dc) between the two buffer pairs;
 *        *result_in_b tells which pair holds d h_init / d c_init; dctx [B,L,H] is ADDED to.
 *        Follow with sf_attn_decoder_wgrad. */
typedef struct sf_follower_episode {
    int32_t S, B, H, D, L, A;
    sf_pano X;
    sf_cands U;
    const float *h_init, *c_init; /* [B,H] */
    const float* ctx;             /* [B,L,H] */
    const uint8_t* ctx_mask;      /* [B,L] */
    sf_decoder_tape tape;
    sf_follower_glue glue;
    sf_dropout drop;              /* p == 0: no dropout */
    uint32_t step0;               /* dropout / sampling site of step 0 */
    /* optional: a second stream.  BACKWARD: with it (and gtape.dcat2 / ds / dh1d) the scoring and
     * text-attention backward of step t-1 run on it while the LSTM / visual backward of step t runs on
     * `stream` (they only meet at the LSTM pointwise backward); the two are ordered with events and the
     * call leaves `stream` behind all of the side stream's work.  FORWARD: ignored -- every forward pass runs on
     * `stream` alone. */
    sf_stream side_stream;
    /* ABI 9, optional, INFERENCE ONLY (drop.p == 0, no backward through this pass: t_text / cat2[:H] / h_tilde of the
     * tape are NOT written; alpha is): two [B,L,H] scratch tensors.  With them sf_follower_episode_fwd forms
     * ctx_q = ctx W_in and ctx_o = ctx W_out[:, :H]^T ONCE (the context is constant over an episode) and runs the text
     * attention of every step but the last in folded form -- scores ctx_q[l] . h1, h~ = tanh(sum alpha_l ctx_o[l] +
     * W_out[:, H:] h1): the same function (fp32 re-association, like q = W_v^T t_v), two dependent launches fewer per
     * decode step.  Needs w->text.w_in_t and w->action.w_a_t; pre-drawn observations or a device-resident environment
     * (glue.nav).  The two fold products run on `stream` in front of step 0's attention. */
    float *ctx_q, *ctx_o;
} sf_follower_episode;
int sf_follower_episode_fwd(const sf_decoder_w* w, const sf_follower_episode* e, void* ws,
                            size_t ws_bytes, sf_stream stream);
int sf_follower_episode_bwd(const sf_decoder_w* w, const sf_follower_episode* e,
                            const sf_decoder_gtape* gtape, const float* gscale, float* dlogit,
                            float* dh_a, float* dc_a, float* dh_b, float* dc_b, float* dctx,
                            int* result_in_b, void* ws, size_t ws_bytes, sf_stream stream);

/* Loss bookkeeping without host syncs or atomics (deterministic order):
 * sum_cnt[t] = (sum_b term[t,b], sum_b live[t,b]) for t < T;  then, optionally after a
 * data-parallel all-reduce of sum_cnt, loss[0] = sum_t sum/cnt (0 where cnt == 0) which is the
 * reference's "sum over steps of per-step means" (follower.py:481, speaker.py:182), and
 * gscale[t] = 1/cnt[t] (0 where cnt == 0) for the backward. */
int sf_reduce_terms(const float* term, const float* live, int T, int B, float* sum_cnt,
                    sf_stream stream);
int sf_loss_finalize(const float* sum_cnt, int T, float* loss, float* gscale, sf_stream stream);

/* ---- EncoderLSTM.forward (model.py:81-104) ----------------------------------------------------
 * seq [B,Lpad] int64 (PAD = 0 after each row's length), lengths [B] int32, T = max length.
 * Packed-sequence semantics: row b advances for t < lengths[b]; ctx [B,T,H] is zero beyond.
 * Writes ctx (dropout site `drop_stream` when training), decoder_init = tanh(W h_T + b), c_T.
 * tape: emb_t [T,B,E], xg [T,B,4H] (hoisted input product), gates [T,B,4H], hs [T+1,B,H],
 * cs [T+1,B,H] (state before/after every step).  An INFERENCE call (no backward to follow) with
 * w->xw_table may pass emb = NULL and gates = NULL: the embedded tokens and the gate tape are then not
 * written (hs / cs are still needed as working storage). */
typedef struct sf_encoder_w {
    const float* embedding; /* [vocab,E] */
    sf_lstm_w lstm;         /* weight_ih_l0 [4H,E] ... */
    const float *w_e2d, *b_e2d; /* encoder2decoder [H,H],[H] */
    const float *w_e2d_t;       /* optional [H,H] transposed */
    /* optional [vocab,4H] = embedding weight_ih_l0^T (refreshed by the host when either changes):
     * the input half of the gates of step t is then the table row of token seq[b,t] -- no
     * [T*B,E]x[E,4H] product, no [T,B,4H] intermediate.  NULL = the product is formed every call. */
    const float* xw_table;
    /* SF_ENC_* bits.  By default, when xw_table is given, H == 512, B <= 128, T <= 128 and the device
     * has >= 256 CUs, the T recurrent steps run as ONE persistent launch (csrc/sf_persist.hip: W_hh in
     * registers, the batch partitioned across the XCDs, h exchanged inside a partition); results are
     * bit-identical to the one-launch-per-step path for B > 16 (same summation order as its
     * 32-row kernel; within 2e-6 of its 16-row kernel below that).  SF_ENC_PER_STEP forces per-step.
     * LIMIT of the per-step path: its kernels cover a reduction of at most 64 chunks of 16, i.e. H <= 1024 (H % 16 == 0);
     * above that sf_encoder_lstm_fwd returns SF_ERR_UNSUPPORTED (tests/test_gpu_lstm_steps.py pins it at H = 1040). */
    int32_t flags;
} sf_encoder_w;
#define SF_ENC_PER_STEP 1
/* The embedding is TRAINABLE (glove=None, model.py:57-60): the reference then also applies its dropout module to
 * the embedded tokens (model.py:86-87), with the probability of `drop` at site drop_stream ^ 0x40000000, keyed on
 * (global row b, column t*E + e).  Needs tape->emb and tape->xg and xw_table == NULL (the input product of dropped
 * embeddings is not a table row). */
#define SF_ENC_EMB_DROPOUT 2
/* One DIRECTION of a bidirectional encoder (model.py:47-66, 92-94: nn.LSTM(bidirectional=True), hidden_size // 2 per
 * direction): the call neither applies encoder2decoder nor tanh -- decoder_init receives the raw h_T, and in the
 * backward d_init is the gradient wrt that raw h_T -- and ctx is written WITHOUT dropout (`drop` then only feeds
 * SF_ENC_EMB_DROPOUT).  The host mirror runs the two directions (the reverse one over per-row reversed tokens),
 * concatenates, drops, and applies encoder2decoder to [h_reverse ; h_forward] itself. */
#define SF_ENC_RAW_STATE 4
/* seq holds every row's tokens in REVERSED order (step t = position lengths[b] - 1 - t): the SF_ENC_EMB_DROPOUT mask is
 * keyed on the position, so that the two directions of a bidirectional encoder drop the same embedded tokens. */
#define SF_ENC_REVERSED 8
/* embedding (optional): gradient of embedding.weight [vocab,E], accumulated: row seq[b,t] += dropout-mask x
 * (dgates[t,b] W_ih); rows of token `padding_idx` receive nothing (nn.Embedding(padding_idx), model.py:55).  Needs
 * seq / Lpad as given to the forward. */
typedef struct sf_encoder_g {
    sf_lstm_g lstm;
    float *w_e2d, *b_e2d;
    float* embedding;
    const int64_t* seq;
    int32_t Lpad, padding_idx;
} sf_encoder_g;
typedef struct sf_encoder_tape { float *emb, *xg, *gates, *hs, *cs; } sf_encoder_tape;
int sf_encoder_lstm_fwd(const sf_encoder_w* w, int B, int Lpad, int T, int E, int H,
                        const int64_t* seq, const int32_t* lengths, float* ctx,
                        float* decoder_init, float* c_t, const sf_encoder_tape* tape,
                        const sf_dropout* drop, uint32_t drop_stream, void* ws, size_t ws_bytes,
                        sf_stream stream);
/* dctx [B,T,H] (gradient wrt the dropped ctx), d_init, d_ct [B,H] in (NULL = zero).  ctx beyond a row's length is the
 * constant 0 (model.py:101), so what dctx holds there is ignored: it reaches no state and no weight gradient. */
int sf_encoder_lstm_bwd(const sf_encoder_w* w, const sf_encoder_g* g, int B, int T, int E, int H,
                        const int32_t* lengths, const float* decoder_init, const float* dctx,
                        const float* d_init, const float* d_ct, const sf_encoder_tape* tape,
                        const sf_dropout* drop, uint32_t drop_stream, void* ws, size_t ws_bytes,
                        sf_stream stream);

/* ---- bidirectional EncoderLSTM (model.py:47-66, 81-104 with bidirectional=True; train.py:197-199) -----------------
 * H = hidden units PER DIRECTION (hidden_size // 2).  fwd / rev: the two directions' weights (weight_ih_l0 ... and
 * weight_ih_l0_reverse ...; their w_e2d fields are ignored), each with its own xw_table; w_e2d / b_e2d [2H,2H],[2H]
 * (w_e2d_t optional) = encoder2decoder.  seq [B,Lpad] in the given token order for both directions: the reverse one reads
 * position lengths[b] - 1 - t at its step t.  Writes
 *   ctx [B,T,2H] = dropout([forward output | reverse output]) (site drop_stream; the mask is keyed on row b and column
 *     t * 2H + j, i.e. it is the mask of sf_dropout_copy over the assembled [B, T * 2H] rows), zero beyond each length;
 *   decoder_init [B,2H] = tanh(encoder2decoder([h_reverse ; h_forward])), c_t [B,2H] = [c_reverse ; c_forward].
 * tape_f / tape_r: each direction's sf_encoder_tape (as for sf_encoder_lstm_fwd, in that direction's step order).
 * With both xw_tables, H == 256, B <= 128, T <= 128, >= 256 CUs and no SF_ENC_PER_STEP in fwd->flags, both recurrences
 * run as ONE persistent launch (16 workgroups per row group and direction); otherwise the entry composes the per-step
 * kernels of sf_encoder_lstm_fwd itself.  path (optional, host): set to 1 when the persistent launch ran, 0 otherwise. */
int sf_encoder_bilstm_fwd(const sf_encoder_w* fwd, const sf_encoder_w* rev, const float* w_e2d, const float* b_e2d,
                          const float* w_e2d_t, int B, int Lpad, int T, int E, int H, const int64_t* seq,
                          const int32_t* lengths, float* ctx, float* decoder_init, float* c_t,
                          const sf_encoder_tape* tape_f, const sf_encoder_tape* tape_r, const sf_dropout* drop,
                          uint32_t drop_stream, int32_t* path, void* ws, size_t ws_bytes, sf_stream stream);
/* dctx [B,T,2H] (gradient wrt the dropped ctx), d_init, d_ct [B,2H] in (NULL = zero); accumulates into g_fwd / g_rev (their
 * w_e2d / b_e2d fields are ignored; embedding gradients: give seq in the FORWARD token order in both -- the entry reverses
 * it for the reverse direction) and g_w_e2d / g_b_e2d (NULL = not needed).  Same persistent condition as the forward
 * (the launch of enc_bwd_persist_kernel for both directions), no embedding gradient; path as there. */
int sf_encoder_bilstm_bwd(const sf_encoder_w* fwd, const sf_encoder_w* rev, const float* w_e2d, const float* w_e2d_t,
                          const sf_encoder_g* g_fwd, const sf_encoder_g* g_rev, float* g_w_e2d, float* g_b_e2d, int B,
                          int T, int E, int H, const int32_t* lengths, const float* decoder_init, const float* dctx,
                          const float* d_init, const float* d_ct, const sf_encoder_tape* tape_f,
                          const sf_encoder_tape* tape_r, const sf_dropout* drop, uint32_t drop_stream, int32_t* path,
                          void* ws, size_t ws_bytes, sf_stream stream);

/* ---- batched feature gathers (env.py:380-383, 771-774, 60-75; follower.py:291-320) ------------
 * Materialise the dense tensors the reference builds on the host, from the HBM table (index form only: X->table,
 * X->loc_table, X->vp, X->view resp. U->table, U->vp, U->cand_view, U->cand_sincos, U->a_num must all be given,
 * SF_ERR_ARG otherwise -- for every one of the four entries below).  Table indices are clamped, never trusted:
 * view[b], cand_view[b,a] into [0, V), a[b] into [0, A); vp < 0 is the zero row.
 * Shapes: the rows move as float4 chunks and the sin/cos part of a candidate row is laid out as four groups of LOC / 16
 * float4, which is the reference's layout (each of sin h, cos h, sin e, cos e repeated LOC / 4 times) only for
 * LOC % 16 == 0.  SF_ERR_UNSUPPORTED, with nothing launched and nothing written, unless
 *     sf_gather_panorama                                                  IMG % 4 == 0 && LOC % 4 == 0
 *     sf_gather_candidates, sf_gather_actions, sf_gather_actions_ld       IMG % 4 == 0 && LOC % 16 == 0
 * for an fp32 table and a binary16 one (sf_feature_table_f16) alike; sf_follower_glue_fwd refuses index-form candidates
 * outside IMG % 4 == 0 && LOC % 16 == 0 in the same way, as the scoring entries and sf_gather_path_actions always have. */
int sf_gather_panorama(const sf_pano* X, int B, float* out /* [B,V,F] */, sf_stream stream);
/* is_valid (optional) [B,A] = a < a_num[b] */
int sf_gather_candidates(const sf_cands* U, int B, float* all_u /* [B,A,F] */,
                         float* is_valid /* [B,A] */, sf_stream stream);
/* rows [B,F] of single chosen actions (speaker.py:104): a <= 0, a >= a_num[b] or vp < 0 => zeros */
int sf_gather_actions(const sf_cands* U, int B, const int32_t* a, float* out, sf_stream stream);
/* The same with a row stride on the output (a multiple of 4, >= F): the previous action's embedding straight into the
 * first half of a decoder step's LSTM input rows (sf_decoder_tape.xin, ld 2F; follower.py:588-590 `u_t_prev`), after which
 * sf_attn_decoder_fwd is called with u_prev = NULL -- one copy launch fewer per search step. */
int sf_gather_actions_ld(const sf_cands* U, int B, const int32_t* a, float* out, int ld_out, sf_stream stream);
/* The chosen-action embeddings of all N = Tp*B (path step, path) pairs of a speaker batch (speaker.py:87-104:
 * `ob['action_embedding'][a]`, zeros for a stop action or a padded step) in one launch: row n of `out` (row stride
 * ld_out floats >= IMG + LOC, so the rows can be the first half of the encoder's LSTM inputs) =
 * table[vp[n], act_view[n]] || [sin h]xg,[cos h]xg,[sin e]xg,[cos e]xg (g = LOC/4; env.py:60-75) where act[n] > 0 and
 * vp[n] >= 0, zeros elsewhere.  table [n_vp,V,IMG]; act_sincos [N,4]. */
int sf_gather_path_actions(const float* table, int V, int IMG, int LOC, const int32_t* vp, const int32_t* act_view,
                           const float* act_sincos, const int32_t* act, int N, float* out, int ld_out,
                           sf_stream stream);

/* ---- speaker (model.py:429-457, 487-519; speaker.py:158-197) ---------------------------------- */
typedef struct sf_spk_decoder_w {
    const float* embedding; /* [vocab,E] */
    sf_lstm_w lstm;         /* LSTMCell(E -> H) */
    sf_softdot_w attn;
    const float *w_out, *b_out; /* decoder2action [vocab,H],[vocab] */
    /* optional [vocab,4H] = embedding W_ih^T, refreshed by the host whenever either changes: the
     * input half of the LSTM gates becomes a row lookup by the previous word (model.py:497 + :515)
     * and the recurrent step is as short as the encoder's.  NULL = multiply every step. */
    const float* xw_table;
    /* SF_SPK_EMB_DROPOUT: the embedding is trainable (glove=None): model.py:499-500 applies dropout to the embedded
     * word in train mode -- site 2*step_id of `drop`; needs tape->emb and xw_table == NULL. */
    int32_t flags;
    /* optional, backward only: decoder2action^T as [H, ldv] (ldv = vocab rounded up to 4, padding columns zero): the
     * gradient wrt h~ = dlogit W_out becomes a K-contiguous product (NULL: the strided NN kernel, 26 us instead of 7). */
    const float* w_out_t;
} sf_spk_decoder_w;
#define SF_SPK_EMB_DROPOUT 1
/* embedding (optional): gradient of embedding.weight [vocab,E], accumulated: row prev_word[b] += mask x (dgates W_ih)
 * (no padding row: model.py:467 builds the speaker's nn.Embedding without padding_idx). */
typedef struct sf_spk_decoder_g { sf_lstm_g lstm; sf_softdot_g attn; float *w_out, *b_out; float* embedding; } sf_spk_decoder_g;
typedef struct sf_spk_decoder_tape {
    float *emb;     /* [B,E] */
    float *gates, *c1, *h1, *cat2, *t_text, *alpha, *h_tilde;
    float *logit;   /* [B,ldv] raw vocabulary logits, ldv = vocab rounded up to 4 */
} sf_spk_decoder_tape;
/* SpeakerDecoderLSTM.forward, non-att-feed branch (model.py:514-518).  prev_word [B] int64. */
int sf_speaker_decoder_fwd(const sf_spk_decoder_w* w, int B, int E, int H, int Tp, int vocab,
                           const int64_t* prev_word, const float* h0, const float* c0,
                           const float* ctx, const uint8_t* ctx_mask, const int32_t* ctx_row,
                           const sf_spk_decoder_tape* tape, const sf_dropout* drop,
                           uint32_t step_id, void* ws, size_t ws_bytes, sf_stream stream);
/* `sample` feedback of the speaker (speaker.py:170-174, D.Categorical(probs).sample()): counter-based draw keyed on
 * (seed, stream, row0 + b) -- csrc/sf_sampling.h; oracle/rng.py mirrors it.  `stream` names the word step (callers
 * pass site + t; sf_speaker_decode uses stream + t for its step t); row0 = global id of local row 0 (data-parallel
 * shards draw what the unsharded batch would).
 * LIMIT: the draw is two-level over ceil(vocab / 32) slots of 32 columns.  vocab <= 1024 (32 slots; the live
 * vocabularies train_vocab.txt 991 and sub_train_vocab.txt 935): the SAME draw in the persistent word loop
 * (sf_speaker_decode) and in the per-step glue (sf_speaker_glue_fwd, sf_speaker_words_fwd).  1025 ... 4096
 * (trainval_vocab.txt: 1 086; sf_speaker_sample_max_vocab()): the per-step glue only -- sf_speaker_decode returns
 * SF_ERR_UNSUPPORTED there for every feedback, as it always has.  Above 4096 feedback 2 is SF_ERR_UNSUPPORTED everywhere.
 * The host classes run `sample` above 1024 only when asked to (SpeakerEngine.wide_sample; NotImplementedError otherwise). */
typedef struct sf_sample {
    uint32_t seed, stream;
    int32_t row0;
    const uint32_t* stream_dev; /* ABI 8, optional: device word added to `stream` (see sf_dropout.site_dev) -- a captured
                                 * `sample` pass draws new words on every replay */
} sf_sample;
/* The WHOLE word loop of an inference pass (speaker.py:158-197: S times SpeakerDecoderLSTM.forward +
 * sf_speaker_glue_fwd, eval mode, no tapes for a backward) as one persistent launch
 * (csrc/sf_persist.hip: weights register-resident, rows partitioned across XCDs, three in-kernel
 * exchanges per word).  targets [S,B] int64; words [S+1,B] with words[0] = the start tokens;
 * feedback 0 = teacher, 1 = argmax, 2 = sample (needs `sample`); step_scores / nll_term / live [S,B] as
 * sf_speaker_glue_fwd;
 * optional outputs (NULL = skip): logits [S,B,ldv], alpha [S,B,Tp], h1_tape / c1_tape [S,B,H].
 * Needs w->xw_table and w->attn.w_in_t.  The attention is evaluated in the folded form
 * cq = ctx W_in, cw = ctx W_c^T (same function, fp32 re-association).  SF_ERR_UNSUPPORTED (H != 512,
 * B > 128, Tp > 12, vocab < 32, vocab > 1024, fewer than 256 CUs; w->xw_table or w->attn.w_in_t missing): run the
 * per-step entry points instead; nothing has been written.  SF_ERR_ARG comes first: feedback outside 0..2, feedback 2
 * without `sample`, one of h1_tape / c1_tape without the other. */
int sf_speaker_decode(const sf_spk_decoder_w* w, int B, int H, int Tp, int vocab, int S, int feedback,
                      int pad_idx, int eos_idx, const int64_t* targets, const float* h_init,
                      const float* c_init, const float* ctx, const uint8_t* ctx_mask, int64_t* words,
                      uint8_t* ended, float* step_scores, float* nll_term, float* live, float* logits,
                      float* alpha, float* h1_tape, float* c1_tape, const sf_sample* sample, void* ws,
                      size_t ws_bytes, sf_stream stream);
/* prev_word [B]: the words the forward embedded (only read when g->embedding is set; NULL otherwise). */
int sf_speaker_decoder_bwd(const sf_spk_decoder_w* w, const sf_spk_decoder_g* g, int B, int E,
                           int H, int Tp, int vocab, const int64_t* prev_word, const float* h0, const float* c0,
                           const float* ctx, const sf_spk_decoder_tape* tape, const float* dlogit,
                           const float* dh1, const float* dc1, float* dh0, float* dc0, float* dctx,
                           const sf_dropout* drop, uint32_t step_id, void* ws, size_t ws_bytes,
                           sf_stream stream);
/* speaker.py:163-191: log-softmax over the vocabulary, NLL terms against target (PAD ignored),
 * next word (feedback 0 = teacher, 1 = argmax, 2 = sample from softmax(logit): needs `sample`, else NULL),
 * score[b] = log p(w_t) (0 if w_t == PAD), ended[b] |= (w_t == EOS).  nll_term/live as in sf_follower_glue_fwd. */
int sf_speaker_glue_fwd(int B, int vocab, int ldv, const float* logit, const int64_t* target,
                        int feedback, int pad_idx, int eos_idx, uint8_t* ended, int64_t* w_t,
                        float* score, float* nll_term, float* live, const sf_sample* sample, sf_stream stream);
/* The widest vocabulary feedback 2 draws over in sf_speaker_glue_fwd / sf_speaker_words_fwd: 4096 (see sf_sample). */
int sf_speaker_sample_max_vocab(void);
/* The speaker's loss from the per-step (NLL sum, live count) table (speaker.py:182, 192-197): the step means are added
 * only up to and including the first step at which EVERY row has produced EOS (the reference leaves its word loop
 * there); gscale[t] = 1 / count for those steps, 0 behind them.  words [T+1,B] as written by the glue / the decode
 * launch (row 0 = start tokens).  T <= 1024. */
int sf_speaker_loss_finalize(const float* sum_cnt, const int64_t* words, int eos_idx, int T, int B, float* loss,
                             float* gscale, sf_stream stream);
int sf_speaker_glue_bwd(int B, int vocab, int ldv, const float* logit, const int64_t* target,
                        int pad_idx, const float* gscale, float* dlogit, sf_stream stream);

/* ---- SpeakerEncoderLSTM.forward (model.py:437-457) in one call: for t in 0..Tp-1: visual attention over the panorama
 * of path step t with the previous hidden state (a1) -> [action embedding | attended feature] -> dropout -> LSTMCell (a2);
 * then decoder_init = tanh(encoder2decoder(h_Tp)).  X0 = the sf_pano of path step 0 of stacked [Tp][B] vp / view index
 * arrays; xin [Tp,B,2F] holds the action embeddings in its first halves on entry (sf_gather_path_actions) unless
 * act_emb [Tp,B,F] is given (train mode: they are dropped into xin here, site 2*(step0+t)); alpha [Tp,B,V], t_v
 * [Tp,B,D], q [Tp,B,F], gates [Tp,B,4H] are the backward's tape; hs, cs [Tp+1,B,H] with row 0 = zeros on entry.
 * ctx [B,Tp,H] (optional, eval mode only: h_t written straight into ctx[:, t]); h_init [B,H].
 * The loop this replaces issued 3 library calls per path step from Python. */
int sf_speaker_encoder_fwd(const sf_visual_w* vw, const sf_lstm_w* lw, const float* w_e2d, const float* b_e2d,
                           const sf_pano* X0, int Tp, int B, int H, int D, float* xin, float* alpha, float* t_v,
                           float* q, float* gates, float* hs, float* cs, float* ctx, const float* act_emb,
                           float* h_init, const sf_dropout* drop, uint32_t step0, void* ws, size_t ws_bytes,
                           sf_stream stream);
/* The visual attention's query through ONE float64 product (inference; ABI 8 addition): M_v = W_v^T W_h [F,H] and
 * c_v = W_v^T b_h [F], formed and kept in float64 by sf_visual_query_fold_f64 (needs w_v_t, w_h_t, b_h; redo it when a
 * weight changes), turn t_v = W_h h + b_h, q = W_v^T t_v (model.py:310-316) into q = M_v h + c_v: one dependent launch
 * fewer per path step and one rounding fewer.  sf_speaker_encoder_fwd_folded is sf_speaker_encoder_fwd with that query
 * (the t_v tape is not written: no backward can follow; `fold` must not be NULL). */
typedef struct sf_visual_fold64 {
    const double* m_v; /* [F,H] */
    const double* c_v; /* [F] */
} sf_visual_fold64;
int sf_visual_query_fold_f64(const sf_visual_w* w, int H, int D, int F, double* m_v, double* c_v, sf_stream stream);
int sf_speaker_encoder_fwd_folded(const sf_visual_fold64* fold, const sf_visual_w* vw, const sf_lstm_w* lw, const float* w_e2d,
                                  const float* b_e2d, const sf_pano* X0, int Tp, int B, int H, int D, float* xin, float* alpha,
                                  float* t_v, float* q, float* gates, float* hs, float* cs, float* ctx, const float* act_emb,
                                  float* h_init, const sf_dropout* drop, uint32_t step0, void* ws, size_t ws_bytes,
                                  sf_stream stream);

/* ---- the speaker's word loop with its tape, in one call each way (speaker.py:158-197 forward, the backward
 * `loss.backward()` of speaker.py:385 walks) -- what a TRAINING iteration runs (sf_speaker_decode keeps no tape):
 * fwd = for t in 0..S-1: sf_speaker_decoder_fwd(words[t], state t-1 -> tape[t], dropout / sampling site step0 + t) then
 *       sf_speaker_glue_fwd(tape[t].logit, targets[t] -> words[t+1], step_scores[t], nll_term[t], live[t]);
 * bwd = for t in S-1..0: sf_speaker_glue_bwd(gscale[t]) then sf_speaker_decoder_bwd, ping-ponging (dh, dc) between the
 *       two buffer pairs; *result_in_b tells which pair holds d h_init / d c_init; dctx [B,Tp,H] is ADDED to.
 * `tape0` holds the pointers of STEP 0 of stacked [S][B][..] tensors (emb may be NULL when nothing will run
 * backward); words [S+1,B] (row 0 = start tokens), targets / step_scores / nll_term / live [S,B], gscale [S].
 * gtape != NULL (needs h0_all [S,B,H]: every step's incoming hidden state, i.e. h_init followed by tape h1 of steps
 * 0..S-2 in ONE array): per step only the DATA gradients are formed and the dY operands kept in the stacked gtape;
 * every weight gradient of `g` is then ONE product over all S*B rows at the end (reduction depth 8 000 instead of
 * 80 products of depth 100 each) -- the follower's scheme (sf_attn_decoder_wgrad).  A trainable embedding
 * (g->embedding) still scatters per step.  dlogit [B,ldv] is scratch and may be NULL with a gtape. */
typedef struct sf_spk_decoder_gtape {
    float *dlogit;   /* [S,B,ldv] */
    float *dpre;     /* [S,B,H]  d(pre-tanh) of attention.linear_out */
    float *dt_text;  /* [S,B,H]  d(linear_in output) */
    float *dgates;   /* [S,B,4H] pre-activation gate gradients */
} sf_spk_decoder_gtape;
int sf_speaker_words_fwd(const sf_spk_decoder_w* w, int B, int E, int H, int Tp, int vocab, int S, int feedback,
                         int pad_idx, int eos_idx, const int64_t* targets, const float* h_init, const float* c_init,
                         const float* ctx, const uint8_t* ctx_mask, int64_t* words, uint8_t* ended, float* step_scores,
                         float* nll_term, float* live, const sf_spk_decoder_tape* tape0, const sf_dropout* drop,
                         uint32_t step0, const sf_sample* sample, void* ws, size_t ws_bytes, sf_stream stream);
int sf_speaker_words_bwd(const sf_spk_decoder_w* w, const sf_spk_decoder_g* g, int B, int E, int H, int Tp, int vocab,
                         int S, int pad_idx, const int64_t* words, const int64_t* targets, const float* h_init,
                         const float* c_init, const float* ctx, const sf_spk_decoder_tape* tape0, const float* gscale,
                         float* dlogit, float* dh_a, float* dc_a, float* dh_b, float* dc_b, float* dctx,
                         int* result_in_b, const sf_dropout* drop, uint32_t step0, const sf_spk_decoder_gtape* gtape,
                         const float* h0_all, void* ws, size_t ws_bytes, sf_stream stream);
/* TEACHER-FORCED pass over S word steps (speaker.py:158-197 with feedback = teacher; ABI 8).  The next input word is
 * the target, so the recurrence does not depend on attention / projection / glue: it runs alone as ONE persistent
 * launch (the encoder's recurrence kernel with a given initial state) and everything else -- dropout(h1), attention over
 * the path context, h~, vocabulary projection, log-soft-max / NLL / score (model.py:516-518, speaker.py:163-191) -- runs
 * for all S*B rows at once.  hs_all / cs_all [S+1,B,H]: slot 0 = the initial state (in), slots 1..S = h1 / c1 of the
 * steps (out; tape0->h1 / c1 must point at slot 1); tape0->gates / cat2 / t_text / alpha / h_tilde / logit are the
 * stacked [S,B,...] tapes of sf_speaker_decoder_fwd (emb optional: all S*B embedded words, for the backward's dW_ih);
 * words [S+1,B] receives words[t+1] = targets[t]; ended / step_scores / nll_term / live as sf_speaker_glue_fwd.
 * Needs w->xw_table, no embedding dropout.  SF_ERR_UNSUPPORTED (H != 512, B > 128, S > 128, < 256 CUs): run
 * sf_speaker_words_fwd. */
int sf_speaker_teacher_fwd(const sf_spk_decoder_w* w, int B, int E, int H, int Tp, int vocab, int S, int pad_idx,
                           int eos_idx, const int64_t* targets, float* hs_all, float* cs_all, const float* ctx,
                           const uint8_t* ctx_mask, int64_t* words, uint8_t* ended, float* step_scores, float* nll_term,
                           float* live, const sf_spk_decoder_tape* tape0, const sf_dropout* drop, uint32_t step0, void* ws,
                           size_t ws_bytes, sf_stream stream);
/* Its backward: the head's backward for all S*B rows at once, the recurrence's backward as one persistent launch with the
 * head's d h1 as per-step external gradient, every weight gradient as ONE product over the stacked rows (g may be NULL:
 * data gradients only).  gscale [S]; dh_init / dc_init [B,H] out (gradient wrt slot 0 of hs_all / cs_all); dctx
 * [B,Tp,H] accumulated; gtape as sf_speaker_words_bwd; dcat2 [S*B,2H], ds [S*B,Tp], dh1_ext [S*B,H]: caller-owned
 * scratch.  SF_ERR_UNSUPPORTED as the forward (and with a trainable embedding): run sf_speaker_words_bwd. */
int sf_speaker_teacher_bwd(const sf_spk_decoder_w* w, const sf_spk_decoder_g* g, int B, int E, int H, int Tp, int vocab,
                           int S, int pad_idx, const int64_t* words, const int64_t* targets, const float* hs_all,
                           const float* cs_all, const float* ctx, const sf_spk_decoder_tape* tape0, const float* gscale,
                           float* dh_init, float* dc_init, float* dctx, const sf_dropout* drop, uint32_t step0,
                           const sf_spk_decoder_gtape* gtape, float* dcat2, float* ds, float* dh1_ext, void* ws,
                           size_t ws_bytes, sf_stream stream);

/* ---- search helpers (follower.py:541-980 beam / state-factored search, speaker.py:211-318) ------
 * dst[i, :width] = src[idx[i], :width] (idx < 0 => zeros): `h_t[flat_indices]`, `c_t[flat_indices]`
 * (follower.py:580, speaker.py:252) as one gather; width, ld_src, ld_dst multiples of 4. */
int sf_gather_rows(const float* src, int ld_src, const int32_t* idx, int n, int width, float* dst,
                   int ld_dst, sf_stream stream);
/* follower.py:585-603 / speaker.py:254-257 on the device: per row of logit [N, ld] (n columns,
 * n <= 1024): columns >= n_valid[row] are set to -inf in place when n_valid is given
 * (`logit[is_valid == 0] = -inf`), then log_softmax, then the k best columns in descending order
 * (ties: lower column first): idx [N,k] int32, logp [N,k] = log_softmax(logit)[row, idx].  k == n
 * returns the whole row sorted (follower.py:802).  idx == NULL (k == n required): no selection -- logp [N,n] =
 * log_softmax(logit) in COLUMN order, -inf beyond n_valid: what state_factored_search consumes (it walks every
 * successor of a state, follower.py:802-836).
 * The order is the stable descending sort of the MASKED row.  Ranks past the finite columns therefore hold the
 * remaining columns in ascending column order with logp = -inf -- the masked columns [n_valid, n) and valid columns
 * whose logit is -inf alike; idx is always a column of [0, n), never -1.  A consumer ends a row's list at the first
 * -inf (or, like sf_follower_beam_select, at the first column that is no candidate of the state).
 * Columns [n, ld) are neither read nor written.  1 <= n_valid[row] is required and every row needs one finite valid
 * column (n_valid is device data and is not checked; a row without one has no log_softmax -- the reference's is NaN
 * there -- and its outputs are undefined).  SF_ERR_ARG for NULL logit / logp, N < 1, n < 1, ld < n, idx == NULL with
 * k != n; SF_ERR_UNSUPPORTED for n > 1024, k < 1, k > n. */
int sf_logprob_topk(float* logit, int ld, int N, int n, const int32_t* n_valid, int k, int32_t* idx,
                    float* logp, sf_stream stream);
/* dst[idx[i], :width] = src[i, :width] (idx < 0: row i skipped): the h / c / attention rows of newly expanded
 * search states into the state pool (the reference keeps them on its InferenceState tuples, follower.py:826-836);
 * width, ld_src, ld_dst multiples of 4; the idx >= 0 must be distinct. */
int sf_scatter_rows(const float* src, int ld_src, const int32_t* idx, int n, int width, float* dst,
                    int ld_dst, sf_stream stream);

/* The speaker's beam selection for one word step (speaker.py:262-296), all instances at once, no host round trip:
 * what search.DeviceSpeakerBeam issues after sf_speaker_decoder_fwd + sf_logprob_topk in its device word loop.
 * R = B * beam_size hypothesis slots; instance b owns slots b*beam_size .. b*beam_size + beam_size - 1, its live slots
 * at the front of that block.  Per instance with inst[b] = (live, n_done, t), live > 0 and t < T (else nothing
 * changes -- steps issued after the search has ended are no-ops):
 *   candidates  score[i] + top_lp[i, j] (float32 add) for the live slots i and their k words j, ordered by score
 *               descending, then flat index i*k + j ascending; the best beam_size are selected (top_w / top_lp are
 *               [R,k] rows of sf_logprob_topk: descending, ties lower column first);
 *   history     selection q goes to position base + p of step t: hist_word / hist_parent (the slot i it extends,
 *               global) / hist_score at [t * ld_hist + base + p]; continuing selections (word != eos, t < T-1) take
 *               p = 0, 1, .. in selection order, finals follow them in selection order; hist_attn (optional, with
 *               alpha [R,Tp]) receives row alpha[i] at [t * ld_hist + i * Tp] for every live slot of the step, i
 *               being the GLOBAL slot b * beam_size + (the slot's place inside its instance) -- the row index of
 *               alpha itself, not the place inside the instance -- so step t's attention rows form an [R,Tp] array
 *               at t * ld_hist whose rows of dead slots are left untouched;
 *   finals      appended to the instance's completion list done_rec / done_score [B, 2*beam_size] in selection order
 *               at n_done, n_done + 1, .. as t * R + base + p (so history row t, position base + p);
 *   next slots  slot base + p (p < live') = continuing selection p: words (int64: the next prev_word), parent (gather
 *               index of its h / c: the slot i of step t) and score; live' = their number, 0 once n_done >= beam_size
 *               (speaker.py:281-290); the other slots get words = eos, parent = -1, score = 0;
 *               inst[b] = (live', n_done + finals, t + 1); live_total[t] += live' (the caller zeroes live_total [T]).
 * A slot's history position at step t is the slot it occupies at step t + 1: the backchain of (t, p) is
 * p -> hist_parent[t, p] = position at t - 1 -> ..., down to the root slot base at t = 0.
 * SF_ERR_ARG on NULL pointers, k < 1, k > beam_size, ld_hist < R (< R * Tp with hist_attn); SF_ERR_UNSUPPORTED for
 * beam_size > 64 (one wavefront per instance, one lane per slot). */
typedef struct sf_spk_beam {
    int32_t B, beam_size, k, T, Tp, eos;
    float* score;         /* [R] running score of every slot */
    int64_t* words;       /* [R] */
    int32_t* parent;      /* [R] */
    int32_t* inst;        /* [B,3] live, n_done, t */
    int32_t* live_total;  /* [T] */
    int32_t *hist_word, *hist_parent;
    float *hist_score, *hist_attn;
    int64_t ld_hist;      /* elements between word steps of every history array */
    int32_t* done_rec;    /* [B, 2*beam_size] */
    float* done_score;    /* [B, 2*beam_size] */
} sf_spk_beam;
int sf_speaker_beam_select(const sf_spk_beam* s, const int32_t* top_w, const float* top_lp, const float* alpha,
                           sf_stream stream);

/* Up to SF_ROW_MOVES_MAX row gathers (scatter = 0: dst[i, :width] = src[idx[i], :width], idx < 0 => zeros) and row
 * scatters (scatter = 1: dst[idx[i], :width] = src[i, :width], idx < 0 => row skipped; the idx >= 0 distinct) over the
 * same n rows in ONE launch: `h_t[flat_indices]` and `c_t[flat_indices]` of a search step (follower.py:588-589, 826-827)
 * together, and the h / c / attention rows of its new states into the state pool together.  width, ld_src, ld_dst
 * multiples of 4.  The moves must not overlap one another. */
#define SF_ROW_MOVES_MAX 4
typedef struct sf_row_move {
    const float* src;
    float* dst;
    const int32_t* idx;
    int32_t ld_src, ld_dst, width;
    int32_t scatter;
} sf_row_move;
int sf_move_rows(const sf_row_move* moves, int n_moves, int n, sf_stream stream);

/* Small utilities used by the host mirror (kept on the stream so rollouts never sync). */
int sf_fill_f32(float* p, size_t n, float v, sf_stream stream);
int sf_add_f32(float* dst, const float* src, size_t n, sf_stream stream); /* dst += src; n > INT_MAX: SF_ERR_UNSUPPORTED */
/* Up to SF_FILL_MAX_REGIONS buffers set to a constant each in ONE launch: the initial conditions of a pass -- zero
 * states (model.py:67-79 init_state, :368 u_begin), the <BOS> word of every row (speaker.py:137), cleared `ended`
 * flags (follower.py:380, speaker.py:136) -- which a host mirror would otherwise issue as one fill per tensor.
 * `count` elements of `width` bytes (1, 4 or 8; ptr aligned to it) are set to the low `width` bytes of `value`
 * (a float travels as its bit pattern).  Regions with count 0 are skipped. */
#define SF_FILL_MAX_REGIONS 8
typedef struct sf_fill_region {
    void* ptr;
    uint64_t count;
    uint64_t value;
    int32_t width;
} sf_fill_region;
int sf_fill_regions(const sf_fill_region* regions, int n, sf_stream stream);
/* dst[b, :N] (row stride ldd) = dropout(src[b, :N]) at site `drop_stream`, columns col0.. */
int sf_dropout_copy(const float* src, int lds, int B, int N, float* dst, int ldd,
                    const sf_dropout* drop, uint32_t drop_stream, int col0, sf_stream stream);
/* dst[C,R] = src[R,C]^T -- builds the transposed weight copies (refresh after each optimizer step) */
int sf_transpose(const float* src, int R, int Ccols, float* dst, sf_stream stream);
/* embedding rows: out[b,:] = table[idx[b],:]  (model.py:497) */
int sf_embedding_fwd(const float* table, int E, const int64_t* idx, int B, float* out,
                     sf_stream stream);

/* ---- a13 the optimizer step (train.py:263-268: optim.Adam(lr=1e-4, weight_decay=5e-4) for the
 * encoder and for the decoder; follower.py:1014-1020 / speaker.py:389-395 call .step() after
 * loss.backward()).  torch.optim.Adam semantics (L2 weight decay added to the gradient, bias
 * correction with the 1-based `step`, no amsgrad) over ONE flat range of n fp32 parameters:
 * p, m (exp_avg), v (exp_avg_sq) are updated in place, g is read.  Hyper-parameters are doubles (as
 * in Python): 1 - beta and the bias corrections are formed in double and rounded to float once.  One launch for a whole
 * optimizer when its parameters, gradients and moments are laid out flat (optim.FusedAdam). */
int sf_adam_step(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int step, sf_stream stream);
/* The same step with its 1-based step counter IN DEVICE MEMORY (ABI 8): `*step_dev` is incremented by the call and the
 * bias corrections are formed from it on the device (double, rounded once, as on the host), so that a hipGraph which
 * captured the call performs step n + 1 on its n-th replay.  coef: 4 floats of device scratch owned by the optimizer.
 * skip_if_nonzero (optional): a device word read on the stream; non-zero turns the call into a no-op (parameters,
 * moments and `*step_dev` untouched).  Given the fault word of the persistent launches (sf_workspace_fault_offset) a
 * captured iteration never steps on gradients a starved launch has poisoned; the host sees the word at its next
 * sync and re-issues the iteration (agents.Seq2SeqAgent.train). */
int sf_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1, double beta2,
                     double eps, double weight_decay, int32_t* step_dev, float* coef, const uint32_t* skip_if_nonzero,
                     sf_stream stream);

/* Development aid (no reference counterpart): while `buf` is non-null, the visual-attention body of
 * the pipelined decode step stamps wall_clock64() (100 MHz) per workgroup into buf[block * 8 + k]
 * (k = 0 start, 1 rows loaded and scored, 2 partials stored); buf = device memory of >= 512 * 8
 * uint64, NULL switches it off.  Used by tools/vis_trace.py to read a kernel's inner timeline. */
void sf_debug_trace(unsigned long long* buf);
/* Development aid: on != 0 makes the persistent launches (csrc/sf_persist.hip) use their
 * placement-independent exchange -- write-through (sc1) stores -- even when a row group's workgroups
 * share an XCD and would keep the exchange inside that XCD's L2.  Lets the tests exercise the protocol
 * the kernels fall back to when the observed workgroup -> XCD placement does not hold. */
void sf_debug_force_write_through(int on);
/* Development aid / test hook: bound of every in-kernel wait of the persistent launches in ticks of 10 ns
 * (< 0 restores the default, 0.25 s).  0 makes the first unsatisfied poll give up: the launch poisons its outputs
 * and raises its fault bit -- how the tests exercise the host's fallback to the per-step kernels. */
void sf_debug_persist_timeout(long long ticks);
/* Test co-tenant: `blocks` workgroups of `threads` threads with `lds_bytes` (<= 65536) of LDS each that stay resident
 * for `ticks` x 10 ns, touching LDS and (sink != NULL: [blocks] floats) a little global memory -- the shape of a
 * collective's channel workgroups (RCCL: a few dozen workgroups of 256-512 threads) -- to be launched on ANOTHER stream
 * beside the persistent launches (tests/test_gpu_cotenancy.py: data-parallel training launches the first gradient
 * bucket's all-reduce beside the persistent encoder backward). */
int sf_debug_cotenant(int blocks, int threads, int lds_bytes, long long ticks, float* sink, sf_stream stream);
/* STRICT summation order for the LSTM gate products (supported runtime switch, round 5).  on != 0: the large gate
 * products (K >= 2048, M <= 128: sf_lstm_cell_fwd, the decode step, the search step) run on the fp32 MFMA
 * (v_mfma_f32_16x16x4_f32, the kernel of rounds 1-3) instead of the bf16 matrix cores with three-way error-free operand
 * splitting.  Both are fp32-accurate (the split form is measured closer to the exact sum); they differ in the last
 * bit or two, and a best-first search that meets two frontier states whose scores are EQUAL to that last bit expands
 * them in the order the arithmetic happens to give.  With the strict order the state-factored search walks the
 * reference's own traversal for 64 of 64 instructions of golden G7b (tests/test_gpu_search.py); the default order
 * re-orders one exact tie (identical completions, order and scores either way).  5.5 us per decode step slower.
 * Process-wide; a captured hipGraph keeps the kernels it was captured with (search.graph_step_for keys its cache on
 * this switch).  sf_gate_product_is_strict() reads it back. */
void sf_gate_product_strict(int on);
int sf_gate_product_is_strict(void);
/* BF16 WEIGHT STORAGE for the LSTM gate product (supported runtime switch, opt-in, additive to ABI 9).
 *
 * Contract: with the switch on, for a REGISTERED weight pair and a SUPPORTED shape, the gate pre-activations that
 * sf_lstm_cell_fwd, the decode step, the search step and sf_linear_slabs_fwd form are the fp32-accurate product of the
 * UNROUNDED activations with bf16_rne(W_ih) and bf16_rne(W_hh) (round to nearest even, bit for bit what
 * torch.Tensor.to(torch.bfloat16) gives): csrc/sf_gemm.hip: gemm_nt_bf16w_kernel reads each weight once per step as ONE
 * bf16 plane (half the bytes of the fp32 rows), keeps the error-free three-way split of the activations, three
 * v_mfma_f32_16x16x32_bf16 per product instead of six.  Biases, the cell and every other product are unchanged.  In every
 * other case -- switch off (the default), pair not registered, shape not supported, strict switch on (it wins) -- the
 * calls run exactly the kernels they run without this feature, bit for bit.  It is an INFERENCE mode: the backward
 * entry points know nothing of it, so a pass whose gradients are wanted must run with the switch off.
 *
 *   sf_pack_bf16_bytes(rows, K)   size of the packed image of a [rows, K] matrix; 0 when K % 64 != 0 or a size is < 1.
 *   sf_pack_bf16(w, ld, rows, K, out, stream)
 *                                 rounds and packs w (fp32, leading dimension ld >= K, ld % 4 == 0, w and out 16-byte
 *                                 aligned) into `out` on `stream`.  The layout is the library's own (opaque).  Call it again
 *                                 (same buffer, in place) whenever the weights change.
 *   sf_lstm_weights_bf16(w_ih, w_hh, packed_ih, packed_hh)
 *                                 associates the fp32 weight ADDRESSES a call will be given (w_hh may be NULL for a product of
 *                                 one segment) with their packed images; both packed pointers NULL forgets the pair.  A few
 *                                 pairs (16) are remembered, under a mutex; SF_ERR_UNSUPPORTED when the table is full.
 *                                 LIFETIME: the caller keeps both packed buffers alive, and their contents current, for as
 *                                 long as the pair is registered and for as long as any captured hipGraph that ran with them
 *                                 may replay -- the library stores the pointers only.
 *   sf_gate_product_bf16_weights(on) / _is_on()
 *                                 the process-wide switch.  A captured hipGraph keeps the kernels (and the packed pointers)
 *                                 it was captured with, whatever the switch says at replay.
 *   sf_gate_product_bf16_supported(M, K1, K2, N)
 *                                 1 when the product x [M,K1] w [N,K1]^T + h [M,K2] u [N,K2]^T takes the bf16 kernel:
 *                                 1 <= M <= 128, K1 > 0 and K1 % 64 == 0, K2 == 0 (no second segment) or K2 % 64 == 0, N >= 1. */
size_t sf_pack_bf16_bytes(int rows, int K);
int sf_pack_bf16(const float* w, int ld, int rows, int K, void* out, sf_stream stream);
int sf_lstm_weights_bf16(const float* w_ih, const float* w_hh, const void* packed_ih, const void* packed_hh);
void sf_gate_product_bf16_weights(int on);
int sf_gate_product_bf16_weights_is_on(void);
int sf_gate_product_bf16_supported(int M, int K1, int K2, int N);
/* FP16 STORAGE for the feature table (opt-in, additive to ABI 9).
 *
 * Contract: a table registered here holds IEEE binary16 [n_viewpoints, V, IMG] (half the bytes of the fp32 table; IMG % 4 ==
 * 0), and every entry point that reads table rows by index -- sf_pano / sf_cands with dense == NULL, forward and backward,
 * the gathers, sf_gather_path_actions -- widens each value to fp32 as it loads it (exact, subnormals included) and then runs
 * the arithmetic of the fp32 kernels: the results are, bit for bit, those of an fp32 table holding the widened values.
 * loc_table, dense sources and every output stay fp32.  The table must hold finite values only (as the fp32 table must).
 * sf_pano and sf_cands keep their layout: the table is known by its ADDRESS, as sf_lstm_weights_bf16 knows weights.
 *
 *   sf_feature_table_f16(table, on)
 *                                 on != 0: the table at this address holds binary16; on == 0 forgets the address (unknown:
 *                                 nothing to do).  A few (16) addresses are remembered, under a mutex; SF_ERR_UNSUPPORTED when
 *                                 full, SF_ERR_ARG on NULL.  An owner of an FP32 table should call it with on == 0 once for
 *                                 its address: an allocator may hand out the address of a freed binary16 table again.
 *                                 LIFETIME: the lookup happens when a call is ENQUEUED (or captured), and selects the kernel.
 *                                 The registration, like the table itself, must therefore outlive every call that names the
 *                                 table and every captured hipGraph that ran with it; a graph keeps the kernels it was
 *                                 captured with, whatever is registered at replay.
 *   sf_feature_table_is_f16(table)
 *                                 1 when the address is registered, else 0.
 * No entry point reads a registered table as fp32 (that would run off its end): each launcher picks the binary16
 * instantiation of its kernel from the source's tag, and returns before launching where it has none. */
int sf_feature_table_f16(const void* table, int on);
int sf_feature_table_is_f16(const void* table);
/* PROJECTED FEATURE TABLES for the inference decode step (opt-in, additive to ABI 9).
 *
 * The decode step dots 36 panorama rows with q = M_v h1 + c_v and up to 16 candidate rows with r = M_a h~ (+ constants;
 * sf_decoder_fold).  Both products only carry the hidden state out to feature space.  In inference the rows are rows of the
 * HBM-resident feature table and the weights are constant, so the association is turned round ONCE per (table, weights):
 *     x . (M_v h1 + c_v) = (x^T M_v) . h1 + x . c_v            u . (M_a h~ + c_a) = (u^T M_a) . h~ + u . c_a
 * and the brackets are rows of four tables.  With F = IMG + LOC, ld = sf_projected_ld(H) = H + 1 rounded up to 4 floats
 * (rows are 16-byte aligned; the padding columns hold zeros):
 *     pv [n_rows, ld]   row n = [x_n^T M_v[:IMG, :] | x_n . c_v[:IMG]]                (n_rows = n_viewpoints * V)
 *     pa [n_rows, ld]   row n = [x_n^T M_a[:IMG, :] | x_n . c_a[:IMG]]
 *     lv [V * V, ld]    the same of the location-embedding table's rows with M_v[IMG:, :], c_v[IMG:]
 *     la [5, ld]        rows 0..3: [sum_{j in block g} M_a[IMG + j, :] | sum_{j in block g} c_a[IMG + j]] for the four
 *                       sin/cos groups of a candidate's location part (each value repeated LOC/4 times, contiguous);
 *                       row 4: [m | c0], the constant row of the scoring fold (m_a row F, c_a[F])
 * A decode step then needs TWO dependent launches behind the LSTM cell instead of four: (1) folded text attention || y
 * || the attention partials of step t + 1 scored from pv / lv and h1; (2) scoring + glue on pa / la with h~ formed in the
 * body || the merge of the partials (sf_debug_projected_partials_late below moves the partials into (2)).  Step 0's
 * attention is one launch from h_init.
 * The products q, t_v', t_a, wt and r are not issued and their tape slots are NOT written.
 *
 * MEMORY AND COST: pv and pa take n_rows * ld * 4 bytes each -- 0.79 GB each (1.57 GB together) for the 10 567 viewpoints
 * of the full R2R table at H = 512 -- and the build is 2 * n_rows * IMG * ld * 2 flop = 1.6 Tflop of fp32-class products
 * (13 ms measured on MI355X).  Worth it for a rollout that is replayed, not for one.
 *
 *   sf_projected_build(fold, table, n_rows, loc_table, V, IMG, LOC, H, pv, pa, lv, la, ws, ws_bytes, stream)
 *                                 fills the four tables from the fold matrices of sf_decoder_fold_build and the fp32 table
 *                                 (SF_ERR_UNSUPPORTED for a table registered as binary16), 16 384 table rows per product,
 *                                 64-bit row offsets, straight into the tables.  IMG % 4 == 0, LOC % 16 == 0, H % 4 == 0.
 *   sf_projected_register(table, p)
 *                                 the tables of `table` (p == NULL forgets the address).  sf_pano / sf_cands keep their
 *                                 layout: like sf_feature_table_f16 the library knows the tables by the table's ADDRESS.
 *                                 One entry per address, 16 addresses, under a mutex.  key_v / key_a name the decoder the
 *                                 tables were built for (sf_visual_w.w_h and sf_scoring_w.w_h): a step of another decoder,
 *                                 another location table or other V / IMG / LOC does not take them.
 *                                 LIFETIME: the lookup happens when a step is ENQUEUED (or captured); the caller keeps the
 *                                 tables alive, and their contents current (rebuild in place when a weight changes), for
 *                                 as long as they are registered and any captured hipGraph that ran with them may replay.
 *   sf_projected_registered(table, out)   1 and *out (optional) when the address is registered, else 0.
 *   sf_projected_use(on) / _is_used()     process-wide switch (default on): off, no step looks the tables up.
 *   sf_projected_steps()                  decode steps issued on the projected chain since the library was loaded (step 0's
 *                                         one-launch head is not a step and is not counted).
 *                                         Both are PROCESS-WIDE: a caller that toggles the switch around a call, or reads the
 *                                         counter before and after it to learn which chain ran, must not have another
 *                                         thread issuing decode steps meanwhile.
 * cand_sincos must be INITIALISED (finite) for every slot of [B, A], padding slots included: the scoring body blends a
 * padded slot's values arithmetically (times 0) where the unprojected kernels select.
 * The chain is taken by sf_follower_episode_fwd only (sf_attn_decoder_tail_fwd has no folded context to hand it), when ALL
 * of these hold, and declines -- before
 * its first launch -- to the chain the step takes today otherwise: the folded text stage applies (inference, ctx_q / ctx_o
 * given); panorama and candidates are index-form rows of the registered fp32 table; the next panorama is known (X_next) or
 * this is the last step; a glue is given; B <= 256. */
typedef struct sf_projected {
    const float *pv, *pa, *lv, *la;
    const float* loc_table;      /* the location-embedding table lv was built from */
    const float *key_v, *key_a;  /* sf_visual_w.w_h, sf_scoring_w.w_h of the decoder the tables belong to */
    int32_t H, ld, V, IMG, LOC, reserved;
} sf_projected;
int sf_projected_ld(int H);
int sf_projected_build(const sf_decoder_fold* fold, const float* table, long long n_rows, const float* loc_table, int V, int IMG,
                       int LOC, int H, float* pv, float* pa, float* lv, float* la, void* ws, size_t ws_bytes,
                       sf_stream stream);
int sf_projected_register(const void* table, const sf_projected* p);
int sf_projected_registered(const void* table, sf_projected* out);
void sf_projected_use(int on);
int sf_projected_is_used(void);
long long sf_projected_steps(void);
/* 1 when a decode step of this shape on index-form fp32 rows can take the projected chain (what a caller asks BEFORE it
 * spends the memory and the build; the step itself still checks its small-product plan and declines if that fails). */
int sf_projected_supported(int B, int H, int L, int A, int V, int IMG, int LOC);
/* Test switch: table rows per product of sf_projected_build (default 16 384; rows <= 0 restores it), so that a build of
 * several chunks -- the 64-bit row offsets between them -- can be checked on a small table. */
void sf_debug_projected_chunk_rows(int rows);
/* GATE-SPACE ROWS for the action half of the decoder LSTM's input (opt-in, additive to ABI 10; rides on the projected chain).
 *
 * A decode step multiplies [u_prev | f | h0] by [W_ih | W_hh]^T.  In the projected inference chain u_prev is the all-zero
 * stop embedding or the candidate row launch (2) of the previous step chose: row (vp, cand_view) of the feature table
 * followed by four sin/cos values, each repeated LOC/4 times (contiguous blocks, the layout `la` above groups by).  The
 * weights are constant during inference, so that half of the product is turned round once per (table, W_ih):
 *     gu [n_rows, 4H]   row n = x_n W_ih[:, 0:IMG]^T                                   (n_rows = n_viewpoints * V)
 *     gl [4, 4H]        row k = sum over block k of the columns W_ih[:, IMG + k LOC/4 .. IMG + (k + 1) LOC/4)
 *     u_prev W_ih[:, 0:F]^T = gu[vp V + cand_view] + sum_k sincos_k gl[k]               (zeros for a zero row)
 * Launch (2) of the projected chain then also writes that [B, 4H] row for the step behind it, whose gate product runs over
 * K = F + H instead of 2 F + H and whose cell kernel adds the row in.  Step 0 keeps the full product, and the raw u_next
 * row is still written (the tape's xin is what it was).
 *
 * MEMORY AND COST: gu takes n_rows * 4H * 4 bytes -- 3.1 GB for the 10 567 viewpoints of the full R2R table at H = 512 --
 * and the build is n_rows * IMG * 4H * 2 flop = 3.2 Tflop of fp32-class products.
 *
 *   sf_gate_rows_build(w_ih, table, n_rows, IMG, LOC, H, gu, gl, ws, ws_bytes, stream)
 *                                 fills both tables from W_ih [4H, 2 (IMG + LOC)] and the fp32 table (SF_ERR_UNSUPPORTED
 *                                 for a table registered as binary16), 16 384 table rows per product (the switch
 *                                 sf_debug_projected_chunk_rows applies), 64-bit row offsets.  IMG % 4 == 0, LOC % 16 == 0,
 *                                 H % 4 == 0.  Never call it inside a stream capture.
 *   sf_gate_rows_register(table, g)
 *                                 the tables of `table` (g == NULL forgets the address): by the feature table's ADDRESS,
 *                                 one entry per address, 16 addresses, like sf_projected_register; key_w names the
 *                                 decoder (sf_lstm_w.w_ih).  Same lifetime rule: alive and current while registered and
 *                                 while a captured hipGraph that ran with them may replay.
 *   sf_gate_rows_registered(table, out)   1 and *out (optional) when the address is registered, else 0.
 *   sf_gate_rows_use(on) / _is_used()     process-wide switch (default on).
 *   sf_gate_rows_steps()                  decode steps whose gate product ran on a gate-space row since the library was loaded.
 * Taken by sf_follower_episode_fwd only, and only TOGETHER with the projected chain: every condition of that chain, the
 * entry's key_w / V / IMG / LOC / H match the step, no dropout, 2 (IMG + LOC) + H > 1024, the bf16 weight storage of the
 * gate product (sf_gate_product_bf16_weights) does not apply to the pair -- its packed images cover the whole W_ih -- and
 * the workspace holds two [B, 4H] rows beside what the steps take.  Otherwise every step launches what it launched
 * without these tables. */
typedef struct sf_gate_rows {
    const float *gu, *gl;
    const float* key_w;          /* sf_lstm_w.w_ih of the decoder the tables belong to */
    int32_t H, V, IMG, LOC;
} sf_gate_rows;
int sf_gate_rows_build(const float* w_ih, const float* table, long long n_rows, int IMG, int LOC, int H, float* gu, float* gl,
                       void* ws, size_t ws_bytes, sf_stream stream);
int sf_gate_rows_register(const void* table, const sf_gate_rows* g);
int sf_gate_rows_registered(const void* table, sf_gate_rows* out);
void sf_gate_rows_use(int on);
int sf_gate_rows_is_used(void);
long long sf_gate_rows_steps(void);
/* GATE-SPACE ROWS for the ATTENDED half of the LSTM input (additive to ABI 10; rides on the rows above and follows their
 * build, use and refresh rules).
 *
 * The other half of the input is the attended feature f = sum_v alpha_v [table[vp, v] | loc[view, v]].  In the projected
 * chain f feeds nothing but the gate product, and the product is linear in f, so its image part is turned round too:
 *     gf [n_rows, 4H]   row n = x_n W_ih[:, F:F+IMG]^T                                  (F = IMG + LOC)
 *     f_img W_ih[:, F:F+IMG]^T = sum_v alpha_v gf[vp V + v]
 * Launch (1)'s attention partials then load gate-space rows where they loaded image rows (4H floats per view: the bytes
 * of an image row at 4H = IMG), their record is (sum of 4H | sum of LOC | scores | m, l), and launch (2)'s merge leaves
 * the normalised 4H part as a [B, 4H] row beside the action half's and the LOC part where it always went
 * (xin[:, F+IMG:2F]).  The location columns W_ih[:, F+IMG:2F] are NOT tabulated: the step behind runs its product over
 * [f_loc | h0], K = LOC + H, and its cell adds both rows.  The image columns xin[:, F:F+IMG] of such a step are not
 * written (nothing reads them: the chain is inference only).  Step 0 keeps the full product.
 *
 * MEMORY AND COST: gf is ANOTHER n_rows * 4H * 4 bytes -- 3.1 GB for the full R2R table at H = 512, beside gu's 3.1 GB --
 * and about 22 ms of build on an MI355X (n_rows * IMG * 4H * 2 flop = 3.2 Tflop).
 *
 *   sf_gate_rows_attended_build(w_ih, table, n_rows, IMG, LOC, H, gf, ws, ws_bytes, stream)
 *                                 fills gf as sf_gate_rows_build fills gu: 16 384 table rows per product
 *                                 (sf_debug_projected_chunk_rows applies), 64-bit row offsets, SF_ERR_UNSUPPORTED for a
 *                                 binary16 table.  Never call it inside a stream capture.
 *   sf_gate_rows_attended_register(table, g) / _registered(table, out)
 *                                 by the feature table's address, like sf_gate_rows_register (g == NULL forgets).
 *   sf_gate_rows_attended_use(on) / _is_used()   process-wide switch (default on).
 *   sf_gate_rows_attended_steps()         decode steps whose cell added an attended row since the library was loaded
 *                                 (each of them also counts in sf_gate_rows_steps, which keeps its meaning).
 *   sf_gate_rows_attended_supported(H, LOC)  1 when launch (1)'s partials take rows of 4H + LOC floats.
 * Taken only where the rows above are taken, and further only with the partials in launch (1)
 * (sf_debug_projected_partials_late off), a row of 4H + LOC floats that their body takes (H <= 512 at LOC = 128), an
 * entry whose key_w / V / IMG / LOC / H match, LOC + H <= 1024, and a workspace that holds two more [B, 4H] rows.
 * Otherwise every step launches what it launched without this table.
 *
 * sf_lstm_cell_rows_fwd is the cell of such a step alone, on caller buffers (tests, tools/gate_rows_attended_ab.py): the product
 * runs over x[:, x_col0:I] and h0, xg (required) and xg2 (optional) are added ahead of the cell.  path 0: what a step
 * takes; 1: the K-split product and the cell kernel (one addend: SF_ERR_UNSUPPORTED with xg2); 2: the fused step kernel
 * (its 32-row x 8-unit form at every B: the 16 x 16 form needs more registers than there are at K = LOC + H = 640). */
typedef struct sf_gate_rows_attended {
    const float* gf;
    const float* key_w;          /* sf_lstm_w.w_ih of the decoder the table belongs to */
    int32_t H, V, IMG, LOC;
} sf_gate_rows_attended;
int sf_gate_rows_attended_build(const float* w_ih, const float* table, long long n_rows, int IMG, int LOC, int H, float* gf,
                                void* ws, size_t ws_bytes, sf_stream stream);
int sf_gate_rows_attended_register(const void* table, const sf_gate_rows_attended* g);
int sf_gate_rows_attended_registered(const void* table, sf_gate_rows_attended* out);
void sf_gate_rows_attended_use(int on);
int sf_gate_rows_attended_is_used(void);
long long sf_gate_rows_attended_steps(void);
int sf_gate_rows_attended_supported(int H, int LOC);
int sf_lstm_cell_rows_fwd(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx, int x_col0, const float* xg,
                          const float* xg2, const float* h0, const float* c0, float* h1, float* c1, float* gates, int path,
                          void* ws, size_t ws_bytes, sf_stream stream);
/* The RECURRENT half of the gates as a row (additive to ABI 10; rides on both tables above).
 *
 * h0 of step t + 1 is h1 of step t, final when step t's cell ends -- two launches before step t + 1's cell starts -- and
 * h0 W_hh^T is 512 of the 640 K columns that cell streams.  So launch (2) of step t also carries the product blocks of
 *     xg_h [B, 4H] = h1 W_hh^T + b_ih + b_hh                     (the small product's body, behind the scoring blocks)
 * and the cell of step t + 1 is a product over f_loc alone (K = LOC) that adds three rows: xg_h, the action half's row and
 * the attended half's.  Step 0 keeps its full product; the last step's launch (2) carries no product blocks.
 *
 *   sf_gate_rows_recurrent_use(on) / _is_used()   process-wide switch (default on); means something only where the
 *                                 attended half's rows are taken.
 *   sf_gate_rows_recurrent_steps()        decode steps whose cell added the recurrent row since the library was loaded
 *                                 (each of them also counts in sf_gate_rows_attended_steps).
 *   sf_gate_rows_recurrent_supported(B, H, LOC)   1 when the attended rows are supported, the cell's rule holds (LOC <= 256,
 *                                 LOC % 4 == 0, H % 8 == 0) and launch (2) takes the plan of [B, H] x [4H, H]^T.
 * Taken only where the attended half's rows are taken and the workspace holds two more [B, 4H] rows: the six rows (each
 * rounded up to 64 floats) must fit an eighth of what the workspace has LEFT once the first four are carved, i.e. 52 rows
 * within the capacity the episode starts with -- B <= 157 or so at H = 512 with a 64 MB workspace; a step
 * whose predecessor did not leave the row takes the K = LOC + H step.  Off, or declined, every step launches what it
 * launched without it: the same kernels and the same bits.
 *
 * sf_lstm_cell_rows3_fwd is that cell alone on caller buffers (tests, tools/recurrent_row_ab.py): xg, xg2 and xg_h are
 * required and 16-byte aligned, xg_h holds the recurrent product AND both biases (w's are not added), the product runs over
 * x[:, x_col0:I]; SF_ERR_UNSUPPORTED where I - x_col0 > 256 or H % 8 != 0.  sf_debug_recurrent_row forms xg_h from h1 on the
 * kernel launch (2) forms it in, with no scoring or merge blocks beside it. */
void sf_gate_rows_recurrent_use(int on);
int sf_gate_rows_recurrent_is_used(void);
long long sf_gate_rows_recurrent_steps(void);
int sf_gate_rows_recurrent_supported(int B, int H, int LOC);
int sf_lstm_cell_rows3_fwd(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx, int x_col0, const float* xg,
                           const float* xg2, const float* xg_h, const float* h0, const float* c0, float* h1, float* c1,
                           float* gates, void* ws, size_t ws_bytes, sf_stream stream);
int sf_debug_recurrent_row(const sf_lstm_w* w, int B, int H, const float* h1, int ldh1, float* xg_h, sf_stream stream);
/* A/B switch of the projected chain: 0 (the default: measured faster, 1.429 against 1.474 ms per headline rollout)
 * puts the attention partials of step t + 1 into launch (1), beside the text stage, and leaves launch (2) their merge;
 * on != 0 puts them into launch (2) (partials, ticket and merge beside the scoring; launch (1) is the text stage and y
 * alone).  A panorama with ceil(IMG / 256) + ceil(LOC / 256) > 9 takes the second placement whatever the switch says. */
void sf_debug_projected_partials_late(int on);
/* Text groups per sample of launch (1) when it carries the attention partials.  The rule (a pure function of B, L and the
 * device): TWO groups of 8 * RPW positions iff the partials ride in the launch, L <= 80 and the four-group grid
 * 3 B + 4 B + product_blocks exceeds `slots`, the workgroups of that launch the device holds at once (CUs x the runtime's
 * occupancy of the four-group kernel: 512 on an MI355X, so B >= 55 at H = 512, where y takes 32 blocks per 16 rows of
 * the batch -- not B >= 69, which counted 32 blocks in all); four groups otherwise.  Every launch adds
 * 4 tickets per sample whatever its count, so launches of both kinds share a workspace.
 * sf_projected_text_groups_plan is the rule alone, no device needed: returns the count (0: bad arguments) and, with
 * `grid`, the launch's block count; product_blocks = blocks of y = W_out[:, H:] h1 (32 x ceil(B / 16) at H = 512: 224 at B = 100); slots 0 = unknown,
 * four groups.  sf_debug_projected_text_groups: 0 the rule (default), 2 or 4 that count wherever it is legal (2: with
 * partials and L <= 80 only) -- for A/B timing and the tests. */
int sf_projected_text_groups_plan(int B, int L, int with_partials, int slots, int product_blocks, int* grid);
void sf_debug_projected_text_groups(int groups);
/* Test entry: the attention of the projected chain's launches (1) and (2) alone, on caller buffers -- the same two kernels
 * with empty text, product and scoring parts, so that panorama shapes no engine is built for (V below 36, tiny rows, small
 * H) reach them.  X: index-form fp32 panorama (V in 19..36); pv [n_vp * V, ld], lv [V * V, ld] as sf_projected_build
 * lays them out (ld % 4 == 0, ld >= H + 1); h1 [B, ldh1]; alpha [B, V]; out [B, ldo], the weighted row sum, no dropout.
 * late == 0: partials in launch (1), merge in launch (2); else partials, ticket and merge in launch (2). */
int sf_debug_projected_attention(const sf_pano* X, int B, int H, const float* pv, const float* lv, int ld, const float* h1,
                                 int ldh1, float* alpha, float* out, int ldo, int late, void* ws, size_t ws_bytes,
                                 sf_stream stream);
/* Older name of the same switch (tools/, A/B timing): on != 0 runs the large LSTM gate products (K >= 2048, M <= 128: sf_lstm_cell_fwd, the decode
 * step) on the fp32 MFMA (v_mfma_f32_16x16x4_f32, rounds 1-3) instead of the bf16 matrix cores with three-way
 * error-free operand splitting (csrc/sf_gemm.hip: gemm_nt_split_kernel; same fp32 accuracy class, measured closer
 * to the exact sum, 6/16 of the matrix-pipe time).  For A/B timing and for the accuracy tests. */
void sf_debug_gate_product_f32(int on);
/* A/B switch (round 5): on == 0 sends the many-row products (M >= 512: the speaker's teacher-forced head over all S*B rows,
 * the beam search's flat steps) back to the register-streaming kernel of rounds 1-4 instead of the LDS-tiled 128 x 128
 * bf16x6 kernel (csrc/sf_gemm.hip: gemm_nt_big_kernel; the default).  Bit 1 of `on` (on == 3) keeps the kernel but turns off
 * the K splits it takes where the consumer sums slabs anyway and the tile count wastes a round of the CUs (the beam
 * step's gate product: 320 tiles -> 3 splits). */
void sf_debug_many_row_product(int on);
/* A/B switch (round 5): on == 0 forms the decoder's small weight gradients one product at a time (two transposes, the
 * many-row product, the slab sum: four dependent launches each) instead of three grouped launches for all of them
 * (csrc/sf_gemm.hip: gemm_tn_group; the default). */
void sf_debug_grouped_weight_gradients(int on);
/* A/B switch (round 5): on == 0 puts the slab-sum launch back between the LSTM's data gradient and the visual-attention
 * backward of a decoder step (the default: the attention backward adds up the K-split slabs of d(feature) itself --
 * same order, same bits). */
void sf_debug_slab_consumers(int on);
/* A/B switch: on == 0 makes sf_speaker_encoder_fwd run its visual attention on the fp32 kernels (rounds 1-4) instead
 * of the float64 query / score path (sf_visual_attention_fwd_f64; the default). */
void sf_debug_precise_attention(int on);
/* Test switch: the weight-gradient products dW += dY^T X whose shape is a whole number of 128 x 128 tiles run as bf16x6
 * split products (gemm_tn_split_kernel) from `rows` reduction rows on (default 4096: where it is faster than the
 * fp32-MFMA kernels; rows < 0 restores the default). */
void sf_debug_tn_split_min_rows(int rows);
/* Byte offset, inside a workspace of `ws_bytes` bytes, of the FAULT WORD (uint32, zero in a healthy process): a
 * persistent launch whose bounded wait gave up (co-residency lost to another process) ORs its bit into it -- 1 encoder
 * forward (sf_encoder_lstm_fwd), 2 encoder backward, 4 speaker word loop (sf_speaker_decode), 8 device-wide lock not
 * obtained -- and poisons its outputs with NaN.  The library never reads or clears the word: the host reads it at a
 * sync it already has, clears it, and re-issues the pass with the per-step kernels (SF_ENC_PER_STEP / the per-step
 * speaker entry points).  speaker_follower_amd.runtime.take_fault does exactly that. */
size_t sf_workspace_fault_offset(size_t ws_bytes);
/* ---- device-resident navigation (env.py:126-146 step, :149-224 panorama sweep, :742-761 teacher,
 * :763-804 observe) ---------------------------------------------------------------------------------
 * The candidate list of a state is a pure function of (viewpoint, view index): the host tabulates it
 * once per connectivity graph (speaker_follower_amd/nav.py) over its own contiguous "nav rows" (one
 * per viewpoint, scans back to back).  State s = nav_row * V + view; candidate a of state s leads to
 * nav row next_row[s,a] facing view cand_view[s,a] (a = 0: stop, next_row = the state's own row). */
typedef struct sf_nav_table {
    const int32_t* a_num;       /* [n_rows*V]      1 + number of neighbours */
    const int32_t* next_row;    /* [n_rows*V, A] */
    const int32_t* cand_view;   /* [n_rows*V, A]   absViewIndex of the candidate = the view after the move */
    const float* cand_sincos;   /* [n_rows*V, A,4] sin/cos of rel_heading, rel_elevation */
    const int32_t* feat_row;    /* [n_rows]        feature-table row of a nav row */
    int32_t A, V;
} sf_nav_table;
/* One env.step + env.observe (+ teacher) for a batch: from state (row[b], view[b]) and the chosen
 * candidate a_t[b] (NULL = no move: the initial observation) to the next state, written as the NEXT
 * decode step's index-form observation (what sf_pano / sf_cands / sf_follower_glue read): row_next,
 * vp_next (feature rows), view_next, a_num_next [B], cand_view_next [B,A], sincos_next [B,A,4] and,
 * when target_next != NULL, the shortest-path teacher action (-1 for rows with ended[b] != 0): the
 * candidate whose next_row equals goal_hop[b, row - hop_base[b]] (the next nav row on the shortest
 * path to the sample's goal, tabulated per sample over its scan's rows), 0 at the goal. */
/* The same step as the tail of the scoring + glue launch (sf_follower_glue.nav): state and outputs as in
 * sf_nav_step; the action and the `ended` flag are the ones the glue has just produced. */
typedef struct sf_nav_io {
    sf_nav_table nav;
    const int32_t *row, *view;   /* [B] current state */
    const int32_t* goal_hop;     /* [B, ld_hop] or NULL with target_next == NULL */
    int32_t ld_hop;
    const int32_t* hop_base;     /* [B] */
    int32_t *row_next, *vp_next, *view_next, *a_num_next; /* [B] */
    int32_t* cand_view_next;     /* [B,A] */
    float* sincos_next;          /* [B,A,4] */
    int64_t* target_next;        /* [B] or NULL */
} sf_nav_io;
int sf_nav_step(const sf_nav_table* nav, int B, const int32_t* row, const int32_t* view,
                const int64_t* a_t, const uint8_t* ended, const int32_t* goal_hop, int ld_hop,
                const int32_t* hop_base, int32_t* row_next, int32_t* vp_next, int32_t* view_next,
                int32_t* a_num_next, int32_t* cand_view_next, float* sincos_next,
                int64_t* target_next, sf_stream stream);
/* sf_nav_walk (csrc/sf_nav.hip; follower.py:197-259, env.py:742-761, 823-848), additive to ABI 10: B whole episodes of
 * a policy that is a table look-up, at most S actions each, in ONE launch.  It leaves a rollout's own arrays -- row /
 * view [S+1,B] (slot 0 = the start state row0 / view0, action t takes slot t to slot t + 1), actions [S,B] -- so that
 * sf_eval_score_routes and DeviceNavBatch.trajectories_from read them as they are, and n_steps [B]: the poses of the
 * RESULT minus one.  The state transition is sf_nav_step's to the letter: s = row * V + view; an action >= a_num[s]
 * counts as 0; action 0, and a candidate whose next_row is the current row, leave the state; otherwise row =
 * next_row[s][a], view = cand_view[s][a].
 *   SF_WALK_STOP      action 0 at t = 0; n_steps = 0.
 *   SF_WALK_SHORTEST  sf_nav_step's teacher: with hop = goal_hop[b][row - hop_base[b]] the action is 0 if hop == row,
 *                     else the first candidate c in [1, a_num) with next_row[s][c] == hop, 0 if there is none.  With k
 *                     the index of the first action 0 (S if there is none) n_steps = min(k, S - 1): the reference
 *                     drops the last observation as the duplicated end state, also when max_steps cut the walk off.
 *   SF_WALK_RANDOM    needs S >= SF_WALK_RANDOM_MOVES + 1.  Action 0 is first_action[b], which must lie in [1, a_num);
 *                     actions 1 .. 4 are 1 and their states must have a_num > 1; action 5 is 0; n_steps = 5.  A row
 *                     that breaks either condition raises err[0], gets n_steps = -1, actions 0 throughout and the
 *                     start state in every slot.
 * After a row's stop its later actions are 0 and its later slots repeat the last state: every element of the four
 * outputs is written by every launch.  first_action is read for SF_WALK_RANDOM only, goal_hop / ld_hop / hop_base for
 * SF_WALK_SHORTEST only (NULL / 0 otherwise).  One wavefront per episode, lane c owns candidate slot c.
 *   SF_ERR_ARG on NULL pointers (of the table: a_num, next_row, cand_view), arrays the policy needs and did not get,
 *   B < 1, S < 1, an unknown policy, SF_WALK_RANDOM with S < 6; SF_ERR_UNSUPPORTED for nav->A > 64; nothing is launched
 *   or written then.  Start rows are the caller's, as for sf_nav_step; a view0 outside [0, V) raises err[0] (only ever
 *   raised) and the row is left as a failed SF_WALK_RANDOM row is, without a look at the table. */
#define SF_WALK_STOP 0
#define SF_WALK_SHORTEST 1
#define SF_WALK_RANDOM 2
#define SF_WALK_RANDOM_MOVES 5
int sf_nav_walk(const sf_nav_table* nav, int policy, int B, int S, const int32_t* row0, const int32_t* view0,
                const int32_t* first_action, const int32_t* goal_hop, int ld_hop, const int32_t* hop_base,
                int32_t* row, int32_t* view, int64_t* actions, int32_t* n_steps, int32_t* err, sf_stream stream);
/* sf_nav_routes (csrc/sf_nav.hip; env.py:742-761, 823-848; speaker.py:68-121), additive to ABI 10: the shortest-path
 * routes of a whole split in ONE launch, either as their lengths or as the speaker's packed index minibatches.  Slot j
 * (0 <= j < n_slots) walks route r = route[j] (route == NULL: r = j) from (row0[r], view0[r]) with SF_WALK_SHORTEST's
 * teacher and sf_nav_step's transition, at most S actions, the stop counted.  The hop comes from ONE table shared by
 * all routes, hop = hop_all[hop_off[r] + (row - hop_base[r])]: hop_all holds, scan after scan, for every goal g of a
 * scan of m rows the m next nav rows towards g (the row itself at the goal and where no path exists), hop_off[r] is
 * the first element of the row of r's goal, hop_base[r] the scan's first nav row and hop_rows[r] its m.  A route stops
 * where hop == row, or where no candidate in [1, a_num) leads to the hop; a candidate that is the current row leaves
 * the state alone.  n = the actions of the walk (1 <= n <= S).
 *   n_actions [n_slots]   n;   reached [n_slots]   1 when the last action is a stop at goal[r], else 0;
 *   rows [S+1, n_slots]   the nav row before action t in slot t (slot 0 = row0[r]), the last row from slot n on.
 * Lengths mode (out == NULL): the three arrays are required.  Pack mode (out != NULL): they are optional (all or none)
 * and hold the same values; slot j is column j % B of minibatch i = j / B (n_slots = M * B), whose block starts at byte
 * mb_off[i] of `out` and has the sections of speaker.packed_layout with (B, Tp = mb_Tp[i], Lmax), each 8-byte aligned,
 * in this order (the gaps between them are not written):
 *   instr_seq  int64 [B, Lmax]  the route's tokens instr_tokens[instr_off[r] .. instr_off[r + 1]) (no tokens given: none)
 *                               cut to Lmax - 1, then `eos` if all of them fit, `pad` behind; where len + 1 > Lmax the
 *                               last column holds token Lmax - 1 instead of eos
 *   vp         int32 [Tp, B]    feat_row of the row before action t;  -1 for t >= n
 *   view       int32 [Tp, B]    the view before action t;              0 for t >= n
 *   act        int32 [Tp, B]    1 for a move, 0 for the stop and for t >= n
 *   act_view   int32 [Tp, B]    cand_view of the chosen slot for a move, else 0
 *   act_sincos float [Tp, B, 4] cand_sincos of the chosen slot for a move, bit for bit; else (0, 1, 0, 1)
 *   path_mask  uint8 [B, Tp]    0 for t < n, 1 behind
 * Every element of every array and section is written by every launch.  mb_Tp / mb_off are HOST arrays: the entry
 * checks them; mb_Tp_dev / mb_off_dev are the same values on the device, which the kernel reads (and checks again: a
 * minibatch whose device values break the rules below raises err[0] and none of its slots is written).
 *   Per slot, each of these raises err[0] (only ever raised) and the slot is written as ONE stop at its start state
 *   (n_actions 1, reached 0, rows = row0[r] throughout): a route index outside [0, N); view0[r] outside [0, V); a row of
 *   the walk, the start row first, whose local index row - hop_base[r] lies outside [0, hop_rows[r]).  Its vp is then
 *   feat_row[row0[r]], or -1 where the route index or the start row itself is at fault (row 0, view 0 for the former).
 *   In pack mode a route with n > mb_Tp[i] raises err[0] too and its column holds one stop at its start; n_actions,
 *   reached and rows still report the walk.
 *   SF_ERR_ARG, with nothing launched or written: NULL nav / io / err, table arrays (a_num, next_row, cand_view; in
 *   pack mode cand_sincos and feat_row too), row0, view0, goal, hop_all, hop_off, hop_base, hop_rows; N < 1, S < 1,
 *   n_slots < 1; lengths mode without its three arrays; pack mode with B < 1, Lmax < 1, M < 1, n_slots != M * B,
 *   out_bytes < 1, a missing mb_* array, only some of n_actions / reached / rows, only one of instr_tokens /
 *   instr_off, mb_Tp[i] outside [1, S], mb_off[i] negative or not a multiple of 8, or a block that would end beyond
 *   out_bytes.  SF_ERR_UNSUPPORTED for nav->A > 64.  One wavefront per slot, lane c owns candidate slot c; no LDS, no
 *   barrier, no atomics. */
typedef struct sf_nav_routes_io {
    int32_t N, S, n_slots;         /* routes of the split; most actions of a route; slots of this launch */
    int32_t B, Lmax, M;            /* pack mode: columns of a minibatch, instruction columns, minibatches */
    int32_t pad, eos;              /* pack mode: the two token ids instr_seq is completed with */
    const int32_t *row0, *view0;   /* [N] start states */
    const int32_t* goal;           /* [N] goal nav rows */
    const int32_t* hop_all;        /* the shared next-hop table */
    const int64_t* hop_off;        /* [N] */
    const int32_t *hop_base, *hop_rows; /* [N] */
    const int32_t* route;          /* [n_slots] or NULL */
    int32_t *n_actions, *reached;  /* [n_slots] */
    int32_t* rows;                 /* [S+1, n_slots] */
    const int32_t* mb_Tp;          /* HOST [M] */
    const int64_t* mb_off;         /* HOST [M] */
    const int32_t* mb_Tp_dev;      /* [M] */
    const int64_t* mb_off_dev;     /* [M] */
    const int64_t* instr_tokens;   /* flat, or NULL */
    const int64_t* instr_off;      /* [N+1], or NULL */
    uint8_t* out;                  /* NULL: lengths mode */
    int64_t out_bytes;
} sf_nav_routes_io;
int sf_nav_routes(const sf_nav_table* nav, const sf_nav_routes_io* io, int32_t* err, sf_stream stream);
/* sf_nav_follower_batches (csrc/sf_nav.hip; env.py:601-626, follower.py:75-105), additive to ABI 10: M FOLLOWER
 * minibatches of B routes each, written in ONE launch in the layout a captured training iteration reads
 * (nav.DeviceNavBatch.pack_layout) -- per minibatch what env._next_minibatch(sort=True) followed by
 * DeviceNavBatch.host_arrays_for(..., fixed=True) forms on the host.  The routes are sf_nav_routes' (row0, view0,
 * hop_all, hop_off, hop_base, hop_rows over N routes; instr_tokens / instr_off, both NULL: every instruction is empty).
 * Slot j (0 <= j < M * B) holds route r = order[j]; minibatch i draws slots i*B .. i*B + B - 1 and its block starts at
 * byte mb_off[i] of `out`.
 *   Sort.  raw[j] = instr_off[r + 1] - instr_off[r], the route's token count (NOT cut to Lmax).  Slot j goes to column
 *   #{j' : raw[j'] > raw[j]} + #{j' < j : raw[j'] == raw[j]} of its minibatch: descending, equal lengths in draw order
 *   (Python's stable sorted(..., reverse=True)).
 *   The block has seven sections, each starting on a 64-byte boundary, in this order (the gaps are not written); column
 *   c holds route r:
 *     seq      int64 [B, Lmax]  the tokens (last first when `reverse`), then `eos`, cut to Lmax, `pad` behind
 *     mask     uint8 [B, Lmax]  1 where the stored id equals `pad`, over the full width
 *     lengths  int32 [B]        min(raw + 1, Lmax)
 *     rows     int32 [B]        row0[r]
 *     views    int32 [B]        view0[r]
 *     hop      int32 [B, ld]    hop_all[hop_off[r] + k] for k < min(hop_rows[r], ld), 0 behind
 *     base     int32 [B]        hop_base[r]
 *   col_route / col_len (int32 [M, B], both or neither): the route index in column c of minibatch i, and `lengths`.
 *   Every element of every section and of col_route / col_len is written by every launch.
 *   Per slot, each of these raises err[0] (only ever raised) and the column holds an empty instruction (seq = eos then
 *   pad, length 1; the slot sorts with raw = 0): a route index outside [0, N) -- rows, views, base and hop are then 0 and
 *   col_route holds the index as given; view0[r] outside [0, V); hop_rows[r] > ld; a last token equal to `eos` (the
 *   host path asserts on it).
 *   mb_off is a HOST array, which the entry checks; mb_off_dev holds the same values on the device, which the kernel
 *   reads (and checks again: a minibatch whose device value breaks the rules raises err[0] and is not written).
 *   SF_ERR_ARG, with nothing launched or written: NULL io / err, row0, view0, hop_all, hop_off, hop_base, hop_rows,
 *   order, mb_off, mb_off_dev, out; N < 1, V < 1, B < 1, Lmax < 1, ld < 1, M < 1; only one of instr_tokens / instr_off,
 *   only one of col_route / col_len; `out` not 8-byte aligned (seq is stored as int64 words); an mb_off[i] that is
 *   negative or not a multiple of 64, or a block that would end beyond out_bytes.  SF_ERR_UNSUPPORTED for B > sf_nav_follower_batches_max_b() (1 024).
 *   One workgroup per minibatch: raw lengths in LDS, a barrier, the slot of every column in LDS, a barrier, then one
 *   wavefront per column with its lanes along Lmax and along ld.  No atomics. */
typedef struct sf_nav_follower_io {
    int32_t N, V;                  /* routes of the set; views of a row (view0 must lie in [0, V)) */
    int32_t B, Lmax, ld, M;        /* columns of a minibatch, instruction columns, hop columns, minibatches */
    int32_t pad, eos, reverse;     /* the two token ids seq is completed with; != 0: last token first */
    const int32_t *row0, *view0;   /* [N] start states */
    const int32_t* hop_all;        /* the shared next-hop table */
    const int64_t* hop_off;        /* [N] */
    const int32_t *hop_base, *hop_rows; /* [N] */
    const int64_t* instr_tokens;   /* flat, or NULL */
    const int64_t* instr_off;      /* [N+1], or NULL */
    const int32_t* order;          /* [M * B] route index of every slot */
    const int64_t* mb_off;         /* HOST [M] */
    const int64_t* mb_off_dev;     /* [M] */
    uint8_t* out;
    int64_t out_bytes;
    int32_t *col_route, *col_len;  /* [M, B] or NULL */
} sf_nav_follower_io;
int sf_nav_follower_batches(const sf_nav_follower_io* io, int32_t* err, sf_stream stream);
int sf_nav_follower_batches_max_b(void);

/* The follower's beam selection for one decode step (follower.py:606-690), all instances at once, no host round trip:
 * what search.DeviceFollowerBeam issues after sf_attn_decoder_fwd + sf_logprob_topk (n_valid = a_num) in its device
 * step loop.  R = B * beam_size hypothesis slots; instance b owns slots b*beam_size .. b*beam_size + beam_size - 1, its
 * live slots at the front of that block.  A slot's state is (row, view) of the navigation table `nav`,
 * sid = row * V + view.  Per instance with inst[b] = (live, n_done, t), live > 0 and t < episode_len (else nothing
 * changes -- steps issued after the search has ended are no-ops):
 *   candidates  for the live slots i and ranks j < k: action top_a[i, j] with score[i] + top_lp[i, j] (float32 add);
 *               top_a / top_lp are [R,k] rows of sf_logprob_topk (descending, ties lower column first).  The first
 *               rank whose action is < 0 or >= a_num[sid] ends slot i's list (is_valid, follower.py:626);
 *   selection   the beam_size best by score descending, then flat index i*k + j ascending; q = 0, 1, .. is the
 *               selection order (the host loop's stable per-instance sort);
 *   successor   of parent state psid under action a: nxt = next_row[psid, a]; the state stays psid when a == 0 or
 *               nxt == psid / V, else it becomes nxt * V + cand_view[psid, a];
 *   history     selection q goes to position base + p of step t: hist_parent (the slot i it extends, global),
 *               hist_action, hist_rank (q), hist_sid (the new state), hist_psid (the parent's state), hist_score at
 *               [t * ld_hist + base + p]; continuing selections (a != 0, t < episode_len - 1) take p = 0, 1, .. in
 *               selection order, finals follow them in selection order; hist_attn (optional, with alpha [R,T])
 *               receives alpha[i] at [t * ld_hist + i * T] for the live slots i.  Positions that hold no selection are
 *               not written (the caller presets hist_action to -1 to tell them apart);
 *   finals      appended to the instance's completion list done_rec / done_score [B, 2*beam_size] in selection order
 *               at n_done, n_done + 1, .. as t * R + base + p;
 *   next slots  slot base + p (p < live') = continuing selection p: row / view [2R] (entries [0, R): the slot's new
 *               state; entries [R, 2R): its parent's state -- both halves are sf_nav_step's input, the second with
 *               act [R] forms the previous action's embedding through sf_gather_actions_ld), parent (gather index of
 *               its h / c: the slot i of step t) and score; live' = their number, 0 once n_done + finals >= beam_size
 *               (follower.py:674); the other slots get act = 0, parent = -1, score = 0 and keep their (valid) state;
 *               inst[b] = (live', n_done + finals, t + 1); live_total[t] += live' (the caller zeroes live_total).
 * A slot's history position at step t is the slot it occupies at step t + 1.  No result of an instance depends on
 * another instance's slots.
 * SF_ERR_ARG on NULL pointers, k < 1, k > beam_size, k > nav.A, ld_hist < R (< R * T with hist_attn);
 * SF_ERR_UNSUPPORTED for beam_size > 64 (one wavefront per instance, one lane per slot). */
typedef struct sf_fol_beam {
    int32_t B, beam_size, k, episode_len, T, reserved;
    sf_nav_table nav;     /* a_num, next_row, cand_view, A, V are read */
    float* score;         /* [R] running score of every slot */
    int32_t *row, *view;  /* [2R] */
    int32_t* act;         /* [R] the action that led to the slot's state (0: none, zero embedding) */
    int32_t* parent;      /* [R] */
    int32_t* inst;        /* [B,3] live, n_done, t */
    int32_t* live_total;  /* [episode_len] */
    int32_t *hist_parent, *hist_action, *hist_rank, *hist_sid, *hist_psid;
    float *hist_score, *hist_attn;
    int64_t ld_hist;      /* elements between steps of every history array */
    int32_t* done_rec;    /* [B, 2*beam_size] */
    float* done_score;    /* [B, 2*beam_size] */
} sf_fol_beam;
int sf_follower_beam_select(const sf_fol_beam* s, const int32_t* top_a, const float* top_lp, const float* alpha,
                            sf_stream stream);

/* One iteration of the state-factored search's bookkeeping (follower.py:783-905; sim/frontier_core.cpp: advance_raw +
 * fill_inputs_raw) for all instances, all state in device memory: what search.DeviceStateFactored issues after
 * sf_attn_decoder_fwd + sf_logprob_topk (column order, k = A) + the scatter of the new states' rows, in its device
 * iteration loop (additive to ABI 9).  A hypothesis ("node") of instance b is row b * node_cap + local of the node
 * arrays, local = 0 (the root), 1, .. in the order the instance creates them: ids do not depend on scheduling.
 *   status      [8] int32: [0] frontier size N, [1] base = pool row of frontier column 0, [2] iterations done, [3] the
 *               overflow flags (SF_SEARCH_OVF_*), rest reserved.  A call with N == 0 or a flag set changes nothing.
 *   inst        [B,8] per instance: number of nodes, of "open" slots, of "held" slots, of completed end states, of
 *               visits, of its frontier columns, the first of its frontier columns (columns are compact and
 *               instance-major: the prefix sum of the counts), the overflow flags it raised.
 *   frontier    [B, successor_size]: the instance's frontier nodes, column order.
 *   dictionaries "open" (states to expand) and "held" (finished hypotheses waiting their turn), each a dense
 *               [B, n_keys] key -> slot table (-1: none) plus slot-ordered key / node / pick [B, slot_cap]; slots are
 *               handed out in insertion order; pick = the entry's score while it waits, -inf once expanded.
 *   successors  of instance b's frontier columns r (node f, state st = node_sid[f]) and actions a < a_num[st]:
 *               score = node_score[f] + logp[(first + r) * ld_logp + a] (float32 add), in descending score, ties in
 *               generation order (r, then a); nxt = next_row[st, a]; the state stays st when a == 0 or nxt == st / V,
 *               else becomes nxt * V + cand_view[st, a]; key = the parent's when it stays, else key_of (key_fields 4:
 *               local_row * V + view; 3: local_row * 12 + view % 12; 2: local_row; 1: 0; local_row = row - base_row[b]);
 *               final = a == 0 or count == episode_len.  Per (key, final) only the first successor in that order may
 *               enter, and does when its dictionary (held if final, else open) holds nothing for the key or a node of
 *               strictly smaller score: a new node (parent f, born = iterations done + 1, pool = base + first + r,
 *               start_pose = the parent's and it stays) replaces / takes the next slot, in that order.
 *   picks       successor_size rounds of first-maximum of pick over open and held (held only when strictly greater;
 *               nothing above -inf: the rounds end); a pick's entry gets pick = -inf.  Held picks complete their key:
 *               comp_node[b, key] = the node (kept if one of no smaller score is there), a first completion appends
 *               the key to comp_order [B, completion_size + successor_size].  Open picks of an instance still below
 *               completion_size form its next frontier and are appended to visits [B, visit_cap].  An instance that
 *               has its completions does nothing.
 *   pack        (second launch, one workgroup) base += N; the counts' prefix sum; dev_in [8, cap] int32 = what
 *               fill_inputs_raw writes for the new frontier: rows nav row, parent's nav row, view, parent's view,
 *               action (0 for a root), pool row, instance, base + column; columns beyond the frontier repeat column 0
 *               with destination -1; an empty frontier pads with instance 0's root and destination -1.
 *   overflow    a capacity that does not hold what an iteration adds (node_cap, slot_cap, visit_cap, a key outside
 *               [0, n_keys), base + N > pool_rows): the flag is set, the frontier emptied (N = 0, padding columns),
 *               nothing is written past a bound; the tables of that search are then unspecified.
 * No workgroup waits for another; every loop is bounded by a capacity.
 * SF_ERR_ARG on NULL pointers, non-positive sizes, key_fields outside 1..4, cap < B * successor_size,
 * ld_logp < nav.A, B * node_cap >= 2^31; SF_ERR_UNSUPPORTED for successor_size * nav.A > 1024 (the successors of an
 * instance are ranked in one workgroup's LDS), successor_size > 64 or B > 256 (one lane per instance in the pack). */
enum {
    SF_SEARCH_OVF_NODES = 1, SF_SEARCH_OVF_SLOTS = 2, SF_SEARCH_OVF_VISITS = 4, SF_SEARCH_OVF_POOL = 8,
    SF_SEARCH_OVF_KEY = 16
};
typedef struct sf_state_search {
    int32_t B, successor_size, completion_size, episode_len, key_fields, n_keys;
    int32_t node_cap, slot_cap, visit_cap, cap, pool_rows, reserved;
    sf_nav_table nav;          /* a_num, next_row, cand_view, A, V are read */
    const int32_t* base_row;   /* [B] first nav row of the instance's scan */
    int32_t* status;           /* [8] */
    int32_t* inst;             /* [B,8] */
    int32_t* frontier;         /* [B, successor_size] */
    int32_t *node_parent, *node_sid, *node_key, *node_action, *node_count, *node_pool, *node_start, *node_born;
    float* node_score;         /* node arrays: [B, node_cap] */
    int32_t *open_slot, *open_key, *open_node;
    float* open_pick;
    int32_t *held_slot, *held_key, *held_node;
    float* held_pick;
    int32_t* comp_node;        /* [B, n_keys], -1: not completed */
    int32_t* comp_order;       /* [B, completion_size + successor_size] */
    int32_t* visits;           /* [B, visit_cap] */
} sf_state_search;
int sf_state_factored_select(const sf_state_search* s, const float* logp, int ld_logp, int32_t* dev_in,
                             sf_stream stream);

/* Scoring of navigation results (tasks/R2R/eval.py:23-139; speaker_follower_amd/evaluation.py), additive to ABI 9.
 *
 * sf_eval_distances: the all-pairs shortest-path distances of n_scans graphs in ONE launch.  A graph is given as the
 * CSR of its IN-edges with nodes in local index order: scan k owns the global nodes node_off[k] .. node_off[k+1] - 1
 * (m_k of them), global node g the edges edge_off[g] .. edge_off[g+1] - 1, edge e comes from LOCAL node edge_src[e]
 * of the same scan with weight edge_w[e] > 0.  The result of scan k is the float64 block D[src][dst], m_k x m_k
 * row-major, at element dist_off[k] of `table`: the fixed point of D[s][s] = 0, D[s][v] = min(D[s][v], min over
 * in-edges (u, v) of D[s][u] + w(u, v)), iterated synchronously from +inf until a round changes nothing -- with
 * positive weights and monotone rounding that system has ONE solution, the numbers a Dijkstra search accumulating
 * d + w outward from s produces, to the last bit.  One float64 add and one compare per edge and
 * round, no fused multiply-add, no re-association; pairs without a path stay +inf.  One wavefront per source, its
 * distance vector (two copies) in LDS; after at most m_k rounds the loop ends, and err[0] is set to 1 if round m_k
 * still changed a value (impossible with positive weights).  err[0] is only ever raised: the caller zeroes it.
 *   n_nodes = node_off[n_scans], max_nodes = the largest m_k (host copies: the launcher sizes the grid from them).
 *   SF_ERR_ARG on NULL pointers, n_scans < 1, n_nodes < 1, max_nodes < 1 or > n_nodes; SF_ERR_UNSUPPORTED, with
 *   nothing launched, for max_nodes > sf_eval_max_nodes() = SF_EVAL_MAX_NODES (512: 8 KB of LDS per source; the
 *   largest R2R scan has 348 viewpoints) -- the caller then computes the scans above the limit on the host and
 *   issues the others.  sf_debug_eval_max_nodes(n) lowers the limit (n in 1..512; anything else restores it), for tests.
 * sf_eval_distances_bytes: the bytes of a table that holds n_scans blocks back to back, 8 * sum of m[k]^2 over the
 *   HOST array m [n_scans]; 0 for NULL, n_scans < 1 or a negative m[k]. */
#define SF_EVAL_MAX_NODES 512
typedef struct sf_eval_graphs {
    int32_t n_scans, n_nodes, max_nodes, reserved;
    const int32_t* node_off;   /* [n_scans + 1] */
    const int32_t* edge_off;   /* [n_nodes + 1] */
    const int32_t* edge_src;   /* [n_edges] local index of the edge's source node */
    const double* edge_w;      /* [n_edges] */
    const int64_t* dist_off;   /* [n_scans] first element of the scan's block in the table */
} sf_eval_graphs;
size_t sf_eval_distances_bytes(const int32_t* m, int n_scans);
int sf_eval_max_nodes(void);
void sf_debug_eval_max_nodes(int n);
int sf_eval_distances(const sf_eval_graphs* g, double* table, int32_t* err, sf_stream stream);
/* sf_eval_score: eval.py:46-84 for the B episodes of a rollout, one thread each.  row [S+1,B] are the nav rows the
 * rollout visited, actions [S,B] what it chose; sample b's scan owns the nav rows scan_base[b] .. scan_base[b] +
 * m[b] - 1 and the block at element dist_off[b] of `table` (local index = row - scan_base[b]).
 *   n             index of the first action 0 (stop) plus 1, else S: the path is row[0..n]
 *   nav_error     D[row[n]][goal_row[b]]
 *   oracle_error  the FIRST minimum of D[row[t]][goal] over t = 0..n (strict <, from t = 0)
 *   length        0.0 + D[row[0]][row[1]] + ... + D[row[n-1]][row[n]], added in path order
 *   steps = n, success = nav_error < margin, oracle_success = oracle_error < margin
 * written at slot[b] of the six arrays ([n_slots]: three float64, three int32); slot[b] == -1 writes nothing.  A row
 * or goal outside its scan, or a slot outside [-1, n_slots), writes nothing and sets err[0] = 1 (only ever raised).
 * SF_ERR_ARG on NULL pointers, S < 1, B < 1, n_slots < 1. */
typedef struct sf_eval_episodes {
    int32_t S, B, n_slots, reserved;
    const int32_t* row;        /* [S+1, B] */
    const int64_t* actions;    /* [S, B] */
    const int32_t* goal_row;   /* [B] nav row of the goal */
    const int32_t* scan_base;  /* [B] */
    const int32_t* m;          /* [B] */
    const int64_t* dist_off;   /* [B] */
    const int32_t* slot;       /* [B] */
    const double* table;
    double margin;
    double *nav_error, *oracle_error, *length;      /* [n_slots] */
    int32_t *steps, *success, *oracle_success;      /* [n_slots] */
} sf_eval_episodes;
int sf_eval_score(const sf_eval_episodes* e, int32_t* err, sf_stream stream);
/* sf_eval_score_routes (csrc/sf_eval_routes.hip; no reference counterpart for the two new values), additive to ABI 9:
 * the six values of sf_eval_score -- the same bits: the first minimum, the length added in path order -- plus the two
 * device quantities of the path-fidelity metrics (SPL, nDTW, SDTW), for B routes in ONE launch,
 * written at slot[b] of eight [n_slots] arrays.  With P = p_0 .. p_n the poses of route b and R = r_0 .. r_{g-1} its
 * gold path:
 *   shortest      D[p_0][r_{g-1}]
 *   dtw           C[n+1][g] of C[0][0] = 0, C[a][0] = C[0][b] = inf otherwise,
 *                 C[a][b] = D[p_{a-1}][r_{b-1}] + min(C[a-1][b], C[a][b-1], C[a-1][b-1])
 * The cost is taken FROM the pose TO the gold node.  A cell is one rounded float64 add of one table element to an exact
 * three-way minimum: the bits do not depend on the order in which the cells are formed (the host runs the rows, the
 * kernel the anti-diagonals).  spl, ndtw and sdtw are formed on the host from these (evaluation.path_metrics_of).
 * Routes are addressed generically: pose t of route b is the nav row row[row_first[b] + t * row_stride], local index =
 * that - scan_base[b]; `row` holds n_rows elements.  n = n_steps[b] when n_steps is given, else derived from actions
 * [S,B] as sf_eval_score does (the first 0 plus one, else S).  Two layouts:
 *   sweep    row [S+1,B] and actions [S,B] as a rollout leaves them: row_stride = B, row_first[b] = b, n_steps = NULL
 *   ragged   the routes back to back in one array: row_stride = 1, row_first = their offsets, n_steps given (routes of
 *            any length: the recurrence runs n + g steps)
 * Gold paths are a ragged table of LOCAL node indices: path k is gold_node[gold_off[k] .. gold_off[k+1]), route b is
 * scored against path gold_id[b], its goal is that path's last node.  scan_base, m, dist_off, slot, table, margin: as
 * in sf_eval_episodes.  One wavefront per route, lane l owns gold position l: SF_EVAL_MAX_GOLD = 64 nodes per gold path
 * (R2R's have at most 7).
 *   SF_ERR_ARG on NULL pointers (n_steps may be NULL; then actions must not be and S >= 1), B, n_slots, row_stride,
 *   n_gold, n_gold_nodes, n_rows or max_gold < 1; SF_ERR_UNSUPPORTED, with nothing launched, for max_gold (a HOST copy
 *   of the longest gold path) > 64 -- the caller then scores on the host.  slot[b] == -1 writes nothing.  A route with
 *   a pose or gold node outside its scan, a pose index outside `row`, a negative step count, a slot outside
 *   [-1, n_slots), a gold_id outside [0, n_gold), a gold path of 0 or more than 64 nodes or outside gold_node, or whose
 *   first pose is not its gold path's first node, writes nothing and sets err[0] = 1 (only ever raised). */
#define SF_EVAL_MAX_GOLD 64
typedef struct sf_eval_routes {
    int32_t S, B, n_slots, row_stride;
    int32_t n_gold, n_gold_nodes, max_gold, reserved;
    int64_t n_rows;            /* elements of `row` */
    const int32_t* row;        /* nav rows */
    const int64_t* row_first;  /* [B] element of pose 0 */
    const int32_t* n_steps;    /* [B], or NULL: from actions */
    const int64_t* actions;    /* [S, B]; read only when n_steps == NULL */
    const int32_t* gold_off;   /* [n_gold + 1] */
    const int32_t* gold_node;  /* [n_gold_nodes] local node indices */
    const int32_t* gold_id;    /* [B] */
    const int32_t* scan_base;  /* [B] */
    const int32_t* m;          /* [B] */
    const int64_t* dist_off;   /* [B] */
    const int32_t* slot;       /* [B] */
    const double* table;
    double margin;
    double *nav_error, *oracle_error, *length, *shortest, *dtw;   /* [n_slots] */
    int32_t *steps, *success, *oracle_success;                   /* [n_slots] */
} sf_eval_routes;
int sf_eval_score_routes(const sf_eval_routes* e, int32_t* err, sf_stream stream);
/* sf_eval_score_routes_coverage (csrc/sf_eval_routes.hip; no reference counterpart), additive to ABI 10: everything
 * sf_eval_score_routes does -- the same launch shape, both layouts, the same eight outputs to the last bit, the same
 * refusals -- plus, in the SAME launch, the one route-dependent part of CLS (coverage weighted by length score;
 * DESIGN.md section 2): per gold node the least distance from any visited pose,
 *   near[slot[b] * near_ld + k] = min over a = 0 .. n of D[p_a][r_k]      for k < g
 * FROM the pose TO the gold node, the direction of dtw's cost.  These are the table elements the warping recurrence
 * loads anyway: lane k folds the cost of each of its cells into a minimum (every (pose, gold node) pair passes there
 * exactly once) and stores its own value.  A minimum is exact, so the bits do not depend on the order.  coverage,
 * length_score and cls are formed on the host from it (evaluation.coverage_metrics_of).  `near` is [n_slots, near_ld];
 * elements k >= g of a row, and the rows of slots no route writes, are not written.
 *   SF_ERR_ARG as sf_eval_score_routes, and for near == NULL or near_ld < max_gold; SF_ERR_UNSUPPORTED likewise.
 *   Every per-route refusal of sf_eval_score_routes, and slot[b] == -1, write nothing to `near` either.  max_gold is a
 *   HOST copy, so the kernel checks the row itself: a route whose gold path has more than near_ld nodes writes nothing
 *   and sets err[0] = 1. */
int sf_eval_score_routes_coverage(const sf_eval_routes* e, double* near, int32_t near_ld, int32_t* err,
                                  sf_stream stream);

/* Scoring of speaker results (tasks/R2R/eval_speaker.py:11-122, tasks/R2R/bleu.py:15-72 and the multi-bleu script it
 * runs; speaker_follower_amd/speaker_evaluation.py), additive to ABI 9.
 *
 * sf_bleu_counts: the ten integers corpus BLEU is a function of, per hypothesis, in ONE launch.  Words are ids of an
 * evaluation-private dictionary 0 .. n_dict - 1 the caller builds BY STRING: every distinct word of the references, of
 * the vocabulary and of the hypotheses has one id, so a reference word outside the vocabulary has an id of its own and
 * cannot match a hypothesis word by accident.  Hypothesis b (b < n_hyps) is scored against the n_refs references of
 * path slot[b]; reference r of slot s is ref_ids[ref_off[s * n_refs + r] .. ref_off[s * n_refs + r + 1]).  Two forms
 * of hypotheses:
 *   packed   words == NULL: hypothesis b is hyp_ids[hyp_off[b] .. hyp_off[b + 1]) (dictionary ids)
 *   matrix   words != NULL: [S, n_hyps] VOCABULARY ids as a decode leaves them, int64 (word_bytes 8) or int16
 *            (word_bytes 2); hypothesis b is column b up to, not including, its first `eos` -- all S words when there is
 *            none, a PAD does not end it (utils.Tokenizer.decode_sentence(break_on_eos=True)) -- each word w (in
 *            [0, n_vocab)) taken through the pair remap[2 w], remap[2 w + 1] to its dictionary ids: (a, -1) one BLEU
 *            word, (a, b) two (train_vocab.txt holds the token '. .', which the script's re-split of the blank-joined
 *            line makes two words), (-1, -1) none (an empty string)
 * rows[slot[b]] = correct_1..4, total_1..4, hyp_len, closest_ref_len (int32 [n_slots, 10]), with for n = 1..4
 *   total_n      the number of n-grams of the hypothesis, max(hyp_len - n + 1, 0)
 *   correct_n    the sum over the DISTINCT n-grams of the hypothesis of min(its count in the hypothesis, the largest
 *                of its counts in the single references)
 *   closest_ref_len  the length of the reference whose length is closest to hyp_len, the SHORTER one on a tie
 * and sums[k] += rows[slot[b]][k] (int64 [10], integer atomics: the order is immaterial; the caller zeroes sums, and
 * gives every slot to at most one hypothesis).  slot[b] == -1 writes nothing.  Anything inconsistent writes nothing
 * and sets err[0] = 1 (only ever raised; the caller zeroes it): a slot outside [-1, n_slots), an id outside the
 * dictionary or the vocabulary, a length above the limits, offsets that decrease.
 * One wavefront per hypothesis, the hypothesis and its references staged in LDS as 16-bit ids: 2 * (SF_BLEU_MAX_HYP +
 * 4) + 2 * SF_BLEU_MAX_REFS * (SF_BLEU_MAX_REF + 4) = 4 648 bytes per wavefront.  An n-gram is the EXACT packing of
 * its up to four 16-bit ids into one 64-bit key -- one compare per pair, no hashing, nothing can collide; lane l owns
 * the start positions l, l + 64, ... of the hypothesis, and a position counts when no earlier position holds the same
 * n-gram.  Integers throughout: bit-equal to speaker_evaluation.bleu_count_rows by construction.
 *   max_hyp, max_ref: HOST copies of the longest hypothesis (matrix form: a bound, S or 2 S where remap holds a
 *   pair; at least S is assumed) and reference.
 *   SF_ERR_ARG on NULL pointers, n_hyps / n_slots / n_refs / n_dict < 1, matrix form with S < 1, n_vocab < 1 or
 *   word_bytes other than 2 and 8; SF_ERR_UNSUPPORTED, with nothing launched, for n_dict > sf_bleu_max_dict() (65 536:
 *   what the key packing holds), a hypothesis above sf_bleu_max_hyp() (256 words; instructions are generated at up to
 *   80), a reference above sf_bleu_max_ref() (512; the longest of the shipped R2R sub-split has 107) or n_refs >
 *   sf_bleu_max_refs() (4) -- the caller then counts those paths on the host.  sf_debug_bleu_limits(dict, hyp, ref,
 *   refs) lowers the limits (each within 1 .. its constant; anything else restores that one), for tests. */
#define SF_BLEU_MAX_DICT 65536
#define SF_BLEU_MAX_HYP 256
#define SF_BLEU_MAX_REF 512
#define SF_BLEU_MAX_REFS 4
typedef struct sf_bleu_batch {
    int32_t n_hyps, n_slots, n_refs, n_dict;
    int32_t max_hyp, max_ref;          /* host copies of the longest hypothesis (packed form) / reference */
    int32_t S, word_bytes, eos, n_vocab; /* matrix form */
    const int32_t* hyp_ids;            /* packed form: [hyp_off[n_hyps]] dictionary ids */
    const int32_t* hyp_off;            /* packed form: [n_hyps + 1] */
    const void* words;                 /* matrix form: [S, n_hyps] vocabulary ids */
    const int32_t* remap;              /* matrix form: [n_vocab, 2] vocabulary id -> its dictionary ids, -1: none */
    const int32_t* ref_ids;            /* [ref_off[n_slots * n_refs]] dictionary ids */
    const int32_t* ref_off;            /* [n_slots * n_refs + 1] */
    const int32_t* slot;               /* [n_hyps] */
    int32_t* rows;                     /* [n_slots, 10] */
    int64_t* sums;                     /* [10] */
} sf_bleu_batch;
int sf_bleu_max_dict(void);
int sf_bleu_max_hyp(void);
int sf_bleu_max_ref(void);
int sf_bleu_max_refs(void);
void sf_debug_bleu_limits(int max_dict, int max_hyp, int max_ref, int max_refs);
int sf_bleu_counts(const sf_bleu_batch* b, int32_t* err, sf_stream stream);

/* Caption metrics next to BLEU (no reference counterpart: ROUGE-L and CIDEr-D as DESIGN.md section 2 defines them over
 * the BLEU words; speaker_follower_amd/speaker_evaluation.py), additive to ABI 10.
 *
 * sf_caption_scores: per hypothesis the PARTS the two metrics are functions of, in ONE launch.  The inputs up to
 * `slot` are those of sf_bleu_batch, member for member: the same dictionary ids, both forms of hypotheses, the same
 * slot, err and refusal conventions and the same limits (the sf_bleu_max getters; sf_debug_bleu_limits lowers them
 * for this entry too).  On top of them one table of unique n-gram keys per order n = 1..4, each sorted ascending, laid
 * one behind the other in `keys` (n_keys1 keys of order 1, then n_keys2 of order 2, ...; an order may hold none) with
 * the float64 idf of every key in `idf` at the same index.  A key is the packing of the n-gram's ids, first word in
 * the lowest 16 bits, the words above the order zero -- which is why the orders have tables of their own: the 2-gram
 * (x, 0) and the 4-gram (x, 0, 0, 0) pack alike.  An n-gram that its table does not hold has idf `idf_miss` (log N
 * of the corpus).  Written per slot s = slot[b], with R = n_refs:
 *   hyp_len[s]        int32    the number of words of the hypothesis
 *   lcs[s * R + j]    int32    the length of the longest common subsequence of the hypothesis and reference j: the
 *                              full dynamic program, a row of it per hypothesis word as a prefix maximum over the wave
 *   hnorm2[s * 4 + n-1]        float64  the sum over the DISTINCT n-grams g of the hypothesis of (tf_h(g) idf(g))^2
 *   dot[(s * R + j) * 4 + n-1] float64  the sum over the same g of min(tf_h(g) idf(g), tf_j(g) idf(g)) * (tf_j(g) idf(g)),
 *                              tf_j the count of g in reference j
 * Sums of non-negative float64 products in an order the kernel is free to choose; the device calls neither log, exp
 * nor sqrt, uses plain stores and no atomics.  The references' norms and lengths and everything else ROUGE-L and
 * CIDEr-D need stay on the host (speaker_evaluation.caption_scores_of).  slot[b] == -1 writes nothing; anything
 * inconsistent writes nothing and raises err[0], as in sf_bleu_counts.
 *   SF_ERR_ARG on NULL pointers, a negative table size and whatever sf_bleu_counts answers it for;
 *   SF_ERR_UNSUPPORTED, with nothing launched, above the limits of sf_bleu_counts. */
typedef struct sf_caption_batch {
    int32_t n_hyps, n_slots, n_refs, n_dict;
    int32_t max_hyp, max_ref;          /* host copies of the longest hypothesis (packed form) / reference */
    int32_t S, word_bytes, eos, n_vocab; /* matrix form */
    const int32_t* hyp_ids;            /* packed form: [hyp_off[n_hyps]] dictionary ids */
    const int32_t* hyp_off;            /* packed form: [n_hyps + 1] */
    const void* words;                 /* matrix form: [S, n_hyps] vocabulary ids */
    const int32_t* remap;              /* matrix form: [n_vocab, 2] vocabulary id -> its dictionary ids, -1: none */
    const int32_t* ref_ids;            /* [ref_off[n_slots * n_refs]] dictionary ids */
    const int32_t* ref_off;            /* [n_slots * n_refs + 1] */
    const int32_t* slot;               /* [n_hyps] */
    int32_t n_keys1, n_keys2, n_keys3, n_keys4;   /* the sizes of the four tables */
    const uint64_t* keys;              /* [n_keys1 + .. + n_keys4] (at least one element: never NULL) */
    const double* idf;                 /* the idf of every key */
    double idf_miss;                   /* the idf of an n-gram outside its table: log N */
    int32_t* hyp_len;                  /* [n_slots] */
    int32_t* lcs;                      /* [n_slots, n_refs] */
    double* dot;                       /* [n_slots, n_refs, 4] */
    double* hnorm2;                    /* [n_slots, 4] */
} sf_caption_batch;
int sf_caption_scores(const sf_caption_batch* b, int32_t* err, sf_stream stream);

/* In-process kernel timing (no reference counterpart; what bench.py's `roofline.kernels` table is
 * measured with).  Between sf_profile_begin() and sf_profile_end() every kernel ANY host thread of the
 * process launches through this library (torch runs backward() on its own thread) carries a start and a stop event on its own dispatch, so a
 * pair's elapsed time is that kernel's execution time on the stream it ran on (the figure rocprofv3
 * --kernel-trace reports).  Not usable during hipGraph stream capture.  sf_profile_end waits for the
 * recorded kernels, writes one text line per kernel name -- "name\tcalls\ttotal_us\tmin_us\tmax_us\n"
 * -- into buf (NUL-terminated, truncated to cap) and returns the bytes the full text needs, or -1. */
int sf_profile_begin(void);
long sf_profile_end(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SF_HIP_H_ */
