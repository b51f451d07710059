// extern "C" entry points of libsf_hip.so (see include/sf_hip.h), first of five units: version, build id, status
// strings, the profiler, the debug setters, the composite operators a1 - a4 and the single-operator entries.  The
// registries are in sf_api_tables.hip, the follower's, encoder's and speaker's sequences in sf_api_follower.hip,
// sf_api_encoder.hip and sf_api_speaker.hip; sf_api_util.h is what they share.  Nothing here allocates or synchronises.
#include "sf_api_util.h"

#include <climits>
#include <map>
#include <string>
#include <vector>

namespace sf {
thread_local hipError_t g_last_hip_error = hipSuccess;

// ---- in-process kernel timing (SF_LAUNCH, sf_common.h) ----
namespace {
struct ProfRec { const char* name; hipEvent_t e0, e1; };
struct Prof {
    std::atomic<bool> active{false};   // read by every SF_LAUNCH on any host thread, flipped by begin / end
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;      // events are created once and reused by later sessions
    size_t used = 0;
};
Prof g_prof;                 // process-wide: torch runs backward() on its own host thread
std::mutex g_prof_mutex;
}  // namespace
bool prof_active() { return g_prof.active.load(std::memory_order_acquire); }
void prof_events(const char* name, hipEvent_t* e0, hipEvent_t* e1) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    Prof& p = g_prof;
    *e0 = *e1 = nullptr;
    if (!p.active.load(std::memory_order_relaxed)) return;     // sf_profile_end won the race: plain launch
    while (p.pool.size() < p.used + 2) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { e = nullptr; }
        p.pool.push_back(e);
    }
    if (!p.pool[p.used] || !p.pool[p.used + 1]) return;        // event creation failed: untimed launch
    *e0 = p.pool[p.used++];
    *e1 = p.pool[p.used++];
    p.recs.push_back(ProfRec{name, *e0, *e1});
}

int g_proj_partials_late = 0;        // sf_debug_projected_partials_late (0: the attention partials in launch (1))

namespace {

constexpr size_t WORKSPACE_BYTES = 64u << 20;
// the weight-gradient entry points take a LARGER scratch buffer when the caller has one (the grouped weight gradients keep
// ~135 MB of transposed operands + slabs); kept apart from the workspace of the decode steps: measured in round 5, a
// 256 MB workspace costs the headline rollout 2 % (1.02 vs 1.04 M agent-steps/s, same kernels, same box)
constexpr size_t WGRAD_WORKSPACE_BYTES = 256u << 20;

int g_slab_consumers = 1;     // sf_debug_slab_consumers: consumers add up K-split slabs themselves (0: a reduce launch in between)

}  // namespace

// ---- a2 LSTMCell --------------------------------------------------------------------------------
int lstm_fwd_i(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx, const float* h0,
               const float* c0, float* h1, float* c1, float* gates, float* h1_drop, int ld_h1_drop,
               const Dropout& drop, Arena ar, hipStream_t st, const float* xg, int x_col0, const float* xg2, int path,
               const float* xg_h) {
    LstmPwFwd p{};
    if (!xg) xg2 = nullptr;
    if (xg_h && !(xg && xg2 && path == 0)) return SF_ERR_UNSUPPORTED;     // (all three rows or none of the third)
    p.xg = xg; p.b_ih = w->b_ih; p.b_hh = w->b_hh;
    p.c0 = c0; p.h0 = h0; p.B = B; p.H = H; p.gates = gates; p.h1 = h1; p.c1 = c1;
    p.h1_drop = h1_drop; p.ld_h1_drop = ld_h1_drop; p.drop = drop; p.lengths = nullptr;
    if (!xg && I + H <= 1024 && H % 16 == 0) {
        // short reduction (speaker decoder LSTMCell(300 -> 512)): one fused launch
        LstmStepArgs f{};
        f.h0 = h0; f.w_hh = w->w_hh; f.x = x; f.ldx = ldx; f.w_ih = w->w_ih; f.I = I; f.xg = nullptr;
        f.b_ih = w->b_ih; f.b_hh = w->b_hh; f.B = B; f.H = H; f.pw = p;
        return lstm_step_fused(f, st);
    }
    if (!xg) x_col0 = 0;
    // all three rows: the recurrent half and the biases are in xg_h, what is left is x[:, x_col0:] alone
    if (xg_h) {
        LstmRowsArgs r{};
        r.x = x + x_col0; r.ldx = ldx; r.w = w->w_ih + x_col0; r.ldw = I; r.K = I - x_col0;
        r.xg_h = xg_h; r.xg = xg; r.xg2 = xg2; r.B = B; r.H = H; r.pw = p;
        return lstm_step_rows(r, st);
    }
    // both halves of the input as gate-space rows: what is left, [x[:, x_col0:] | h0], is a short reduction again
    if (xg && (path == 2 || (path == 0 && xg2 && short_gate_fused(I - x_col0, H)))) {
        LstmStepArgs f{};
        f.h0 = h0; f.w_hh = w->w_hh; f.x = x + x_col0; f.ldx = ldx; f.w_ih = w->w_ih + x_col0; f.ld_w_ih = I;
        f.I = I - x_col0; f.xg = xg; f.xg2 = xg2; f.wide = true;
        f.b_ih = w->b_ih; f.b_hh = w->b_hh; f.B = B; f.H = H; f.pw = p;
        return lstm_step_fused(f, st);
    }
    if (xg2) return SF_ERR_UNSUPPORTED;      // (the cell kernel behind the product has one addend; nothing was launched)
    Seg segs[2] = {{x + x_col0, ldx, w->w_ih + x_col0, I, I - x_col0}, {h0, H, w->w_hh, H, H}};
    LinearOut o{};
    float* slabs = nullptr;
    int ks = 1;
    const void* packed[2];
    const bool bf16w = !xg && bf16_packed(w->w_ih, w->w_hh, packed);     // (the packed images cover the whole W_ih)
    TRY(linear_nt(segs, 2, B, 4 * H, o, ar.rest(), ar.rest_n(), st, &slabs, &ks, bf16w ? packed : nullptr));
    p.slabs = slabs; p.ks = ks;
    return lstm_pointwise_fwd(p, st);
}

int lstm_bwd_i(const sf_lstm_w* w, const sf_lstm_g* g, int B, int I, int H, const float* x, int ldx,
               const float* h0, const float* c0, const float* c1, const float* gates,
               const float* dh1, const float* dh1_b, const float* dc1, float* dx, int lddx,
               float* dh0, float* dc0, Arena ar, hipStream_t st, float* dgates_out, int dx_col0,
               const Dropout* dh1b_drop, SmallPlan* dh0_plan, bool* dh0_deferred,
               const float** dx_slabs, int* dx_ks) {   // (with dx_col0 > 0) leave d(x[:, dx_col0:]) as the
    // K-split slabs of its product: *dx_slabs -> [*dx_ks][B, I - dx_col0] (the consumer adds them up: one launch fewer);
    // *dx_ks == 0: dx was formed as usual
    // dh0_plan: do not launch dh0 = dgates W_hh; hand its launch plan to the caller (who pairs it with
    // an independent kernel) when the short-reduction kernel covers the shape
    float* dgates = dgates_out ? dgates_out : ar.take((size_t)B * 4 * H);
    NEED(dgates);
    // the cell's pointwise backward (no packed-sequence or ctx terms)
    LstmPwBwd p{};
    p.gates = gates; p.c0 = c0; p.c1 = c1; p.dh1 = dh1; p.dh1_b = dh1_b; p.dc1 = dc1;
    p.B = B; p.H = H; p.dgates = dgates; p.dc0 = dc0; p.lengths = nullptr; p.dh0_pass = nullptr;
    if (dh1b_drop) p.dh1b_drop = *dh1b_drop;
    TRY(lstm_pointwise_bwd(p, st));
    if (dx && dx_col0 == 0) {
        TRY(data_grad(dgates, 4 * H, w->w_ih, w->w_ih_t, B, 4 * H, I, dx, lddx, 0, ar, st));
    } else if (dx) {
        const int I2 = I - dx_col0;
        if (dx_ks) *dx_ks = 0;
        if (w->w_ih_t) {
            Seg sg{dgates, 4 * H, w->w_ih_t + (size_t)dx_col0 * 4 * H, 4 * H, 4 * H};
            LinearOut o{};
            o.y = dx + dx_col0; o.ldy = lddx; o.epi = EPI_NONE;
            float* slabs = (dx_slabs && dx_ks && g_slab_consumers) ? ar.take((size_t)16 * B * I2) : nullptr;
            int ks = 0;
            float* raw = nullptr;
            if (slabs && linear_nt(&sg, 1, B, I2, o, slabs, (size_t)16 * B * I2, st, &raw, &ks) == SF_OK && raw == slabs && ks >= 1) {
                *dx_slabs = slabs;
                *dx_ks = ks;
            } else {
                TRY(linear_nt(&sg, 1, B, I2, o, ar.rest(), ar.rest_n(), st));
            }
        } else {
            TRY(gemm_nn_ws(dgates, 4 * H, w->w_ih + dx_col0, I, B, I2, 4 * H, dx + dx_col0, lddx, 0,
                           ar.rest(), ar.rest_n(), st));
        }
    }
    if (dh0_deferred) *dh0_deferred = false;
    if (dh0 && dh0_plan && dh0_deferred && w->w_hh_t) {
        Seg sg{dgates, 4 * H, w->w_hh_t, 4 * H, 4 * H};
        LinearOut o{};
        o.y = dh0; o.ldy = H; o.epi = EPI_NONE;
        *dh0_deferred = linear_small_plan(&sg, 1, B, H, o, dh0_plan);
    }
    if (dh0 && !(dh0_deferred && *dh0_deferred))
        TRY(data_grad(dgates, 4 * H, w->w_hh, w->w_hh_t, B, 4 * H, H, dh0, H, 0, ar, st));
    if (g) {
        if (g->w_ih) TRY(gemm_tn(dgates, 4 * H, x, ldx, B, 4 * H, I, g->w_ih, I, 1, st, ar.rest(), ar.rest_n()));
        if (g->w_hh) TRY(gemm_tn(dgates, 4 * H, h0, H, B, 4 * H, H, g->w_hh, H, 1, st, ar.rest(), ar.rest_n()));
        TRY(colsum_pair(dgates, 4 * H, B, 4 * H, g->b_ih, g->b_hh, ar, st));
    }
    return SF_OK;
}

// ---- a1 VisualSoftDotAttention ---------------------------------------------------------------------
int visual_fwd_i(const sf_visual_w* w, const PanoSrc& X, int B, int H, int D, const float* h,
                 float* out, int ldo, float* alpha, float* t_v, float* q, const Dropout& drop,
                 int col0, Arena ar, hipStream_t st, bool precise, const sf_visual_fold64* fold64) {
    const int F = X.IMG + X.LOC;
    if (precise && fold64 && fold64->m_v && fold64->c_v && visual_attn_f64_supported(X, B) && !(H & 3)) {
        // inference through the float64 fold: q = M_v h + c_v in ONE product (t_v is not formed: no backward follows)
        double* q64 = reinterpret_cast<double*>(ar.take((size_t)B * F * 2));
        float* part = ar.take(visual_attn_split_floats(B, F));
        if (q64 && part && ar.tickets()) {
            TRY(linear_f64_w64(h, H, fold64->m_v, H, fold64->c_v, B, F, H, q64, F, q, F, st));
            return visual_attn(0, X, B, q, F, alpha, out, ldo, drop, col0, st, part, ar.tickets(), q64);
        }
    }
    if (precise && w->w_v_t && visual_attn_f64_supported(X, B) && !(H & 3) && !(D & 3)) {
        // The speaker's path encoder (csrc/sf_precise.hip): t_v, q and the scores in float64 -- each intermediate is
        // rounded ONCE.  t_v / q also land in their fp32 tapes (the backward reads those).
        double* t64 = reinterpret_cast<double*>(ar.take((size_t)B * D * 2));
        double* q64 = reinterpret_cast<double*>(ar.take((size_t)B * F * 2));
        float* part = ar.take(visual_attn_split_floats(B, F));
        if (t64 && q64 && part && ar.tickets()) {
            TRY(linear_f64(h, nullptr, H, w->w_h, H, w->b_h, B, D, H, t64, D, t_v, D, st));
            TRY(linear_f64(nullptr, t64, D, w->w_v_t, D, nullptr, B, F, D, q64, F, q, F, st));
            return visual_attn(0, X, B, q, F, alpha, out, ldo, drop, col0, st, part, ar.tickets(), q64);
        }
    }
    TRY(linear_plain(h, H, w->w_h, H, w->b_h, B, D, H, EPI_NONE, t_v, D, ar, st));
    if (w->w_v_t)   // q = t_v W_v as a K-contiguous product against the transposed copy
        TRY(linear_plain(t_v, D, w->w_v_t, D, nullptr, B, F, D, EPI_NONE, q, F, ar, st));
    else
        TRY(gemm_nn_ws(t_v, D, w->w_v, F, B, F, D, q, F, 0, ar.rest(), ar.rest_n(), st));
    // (the products above are done with their slabs by the time the attention kernel runs: the
    // partials may reuse that part of the workspace)
    float* part = B <= 1024 ? ar.take(visual_attn_split_floats(B, F)) : nullptr;
    return visual_attn(0, X, B, q, F, alpha, out, ldo, drop, col0, st, part,
                       part ? ar.tickets() : nullptr);
}

int visual_bwd_i(const sf_visual_w* w, const sf_visual_g* g, const PanoSrc& X, int B, int H, int D,
                 const float* h, const float* alpha, const float* t_v, const float* dout, int lddo,
                 const Dropout& drop, int col0, float* dh, Arena ar, hipStream_t st,
                 float* dq_out, float* dt_out, const SmallPlan* beside, int dout_slabs, long dout_slab_stride) {
    const int F = X.IMG + X.LOC;                        // the attention backward (must run either way)
    float* dq = dq_out ? dq_out : ar.take((size_t)B * F);
    float* dt = dt_out ? dt_out : ar.take((size_t)B * D);
    NEED(dq && dt);
    bool paired = false;
    if (beside) {
        const int rc = pair_visbwd_small(X, B, dout, lddo, const_cast<float*>(alpha), dq, F, drop, col0,
                                         *beside, st, dout_slabs, dout_slab_stride);
        if (rc == SF_OK) paired = true;
        else if (rc != SF_ERR_UNSUPPORTED) return rc;
        else TRY(launch_small_plan(*beside, st));
    }
    if (!paired) TRY(visual_attn(1, X, B, dout, lddo, const_cast<float*>(alpha), dq, F, drop, col0, st, nullptr, nullptr,
                                 nullptr, dout_slabs, dout_slab_stride));
    TRY(linear_plain(dq, F, w->w_v, F, nullptr, B, D, F, EPI_NONE, dt, D, ar, st));
    if (g && g->w_v) TRY(gemm_tn(t_v, D, dq, F, B, D, F, g->w_v, F, 1, st, ar.rest(), ar.rest_n()));
    // g->b_v: the bias shifts all V scores of a row equally; its gradient is identically zero.
    if (dh) TRY(data_grad(dt, D, w->w_h, w->w_h_t, B, D, H, dh, H, 1, ar, st));
    if (g && g->w_h) TRY(gemm_tn(dt, D, h, H, B, D, H, g->w_h, H, 1, st, ar.rest(), ar.rest_n()));
    if (g && g->b_h) TRY(colsum(dt, D, B, D, g->b_h, 1, st, nullptr, ar.rest(), ar.rest_n()));
    return SF_OK;
}

// ---- a3 SoftDotAttention ----------------------------------------------------------------------------
int softdot_fwd_i(const sf_softdot_w* w, int B, int L, int H, const float* copy_from, int ldh,
                  const float* ctx, const uint8_t* mask, float* h_tilde, float* alpha, float* cat2,
                  float* t_text, Arena ar, hipStream_t st, const int32_t* ctx_row) {
    if (copy_from) {
        Dropout none = make_dropout(nullptr, 0);
        TRY(dropout_copy(copy_from, ldh, B, H, cat2 + H, 2 * H, none, 0, st));
    }
    TRY(linear_plain(cat2 + H, 2 * H, w->w_in, H, nullptr, B, H, H, EPI_NONE, t_text, H, ar, st));
    TRY(text_attn_fwd(ctx, mask, B, L, H, t_text, H, alpha, cat2, 2 * H, st, ctx_row));
    return linear_plain(cat2, 2 * H, w->w_out, 2 * H, nullptr, B, H, 2 * H, EPI_TANH, h_tilde, H, ar,
                        st);
}

int softdot_bwd_i(const sf_softdot_w* w, const sf_softdot_g* g, int B, int L, int H,
                  const float* ctx, const float* alpha, const float* cat2, const float* t_text,
                  const float* h_tilde, const float* dh_tilde, float* dh, int lddh, float* dctx,
                  Arena ar, hipStream_t st, float* dpre_out, float* dt_out, bool dpre_ready,
                  float* dcat2_out, float* ds_out, const int32_t* ctx_row) {
    float* dpre = dpre_out ? dpre_out : ar.take((size_t)B * H);
    float* dt = dt_out ? dt_out : ar.take((size_t)B * H);
    float* dcat2 = dcat2_out ? dcat2_out : ar.take((size_t)B * 2 * H);
    const bool defer = dcat2_out && ds_out;
    NEED(dpre && dcat2 && dt);
    if (dpre_ready) dpre = const_cast<float*>(dh_tilde);
    else TRY(tanh_bwd(h_tilde, H, dh_tilde, H, B, H, dpre, H, st));
    TRY(data_grad(dpre, H, w->w_out, w->w_out_t, B, H, 2 * H, dcat2, 2 * H, 0, ar, st));
    if (g && g->w_out) TRY(gemm_tn(dpre, H, cat2, 2 * H, B, H, 2 * H, g->w_out, 2 * H, 1, st, ar.rest(), ar.rest_n()));
    TRY(text_attn_bwd(ctx, B, L, H, dcat2, 2 * H, t_text, H, alpha, dt, H, defer ? nullptr : dctx, st,
                      defer ? ds_out : nullptr, ctx_row));
    // dh = dcat2[:, H:] + dt W_in: the addend rides in the epilogue of the product
    bool dh_done = false;
    if (w->w_in_t) {
        Seg sg{dt, H, w->w_in_t, H, H};
        LinearOut o{};
        o.y = dh; o.ldy = lddh; o.epi = EPI_NONE; o.addend = dcat2 + H; o.ld_addend = 2 * H;
        const int rc = linear_nt(&sg, 1, B, H, o, ar.rest(), ar.rest_n(), st);
        if (rc == SF_OK) dh_done = true;
        else if (rc != SF_ERR_UNSUPPORTED) return rc;
    }
    if (!dh_done) {
        TRY(add2(dcat2 + H, 2 * H, nullptr, 0, B, H, dh, lddh, st));
        TRY(data_grad(dt, H, w->w_in, w->w_in_t, B, H, H, dh, lddh, 1, ar, st));
    }
    if (g && g->w_in) TRY(gemm_tn(dt, H, cat2 + H, 2 * H, B, H, H, g->w_in, H, 1, st, ar.rest(), ar.rest_n()));
    return SF_OK;
}

// ---- a4 EltwiseProdScoring --------------------------------------------------------------------------
int scoring_fwd_i(const sf_scoring_w* w, const CandSrc& U, int B, int H, int D, const float* h,
                  float* logit, float* t_a, float* wt, float* r, Arena ar, hipStream_t st,
                  const sf_follower_glue* glue, bool t_a_done) {
    const int F = U.IMG + U.LOC;
    Seg sg{h, H, w->w_h, H, H};
    LinearOut o{};
    o.y = wt; o.ldy = D; o.bias = w->b_h; o.mul = w->w_out; o.y_pre = t_a; o.ldy_pre = D;
    o.epi = EPI_MUL;
    if (!t_a_done) TRY(linear_nt(&sg, 1, B, D, o, ar.rest(), ar.rest_n(), st));
    if (w->w_a_t)
        TRY(linear_plain(wt, D, w->w_a_t, D, nullptr, B, F, D, EPI_NONE, r, F, ar, st));
    else
        TRY(gemm_nn_ws(wt, D, w->w_a, F, B, F, D, r, F, 0, ar.rest(), ar.rest_n(), st));
    if (glue) return score_glue_fwd(U, B, D, r, wt, w->b_a, w->b_out, make_glue(U, B, logit, glue), st);
    return score_fwd(U, B, D, r, wt, w->b_a, w->b_out, logit, st);
}

int scoring_bwd_i(const sf_scoring_w* w, const sf_scoring_g* g, const CandSrc& U, int B, int H,
                  int D, const float* h, const float* t_a, const float* wt, const float* dlogit,
                  float* dh, Arena ar, hipStream_t st, const sf_decoder_gtape* gt,
                  const float* tanh_of, bool* tanh_done, const CeSrc* ce) {
    // tanh_of (= h, the tanh output that fed the scoring): when given and the shape allows, dh is
    // returned already multiplied by (1 - tanh_of^2) and *tanh_done is set
    const int F = U.IMG + U.LOC;
    float* dr = gt ? gt->dr : ar.take((size_t)B * F);
    float* dc = gt ? gt->dc : ar.take((size_t)B);
    float* dwt = gt ? gt->dwt : ar.take((size_t)B * D);
    float* dta = gt ? gt->dta : ar.take((size_t)B * D);
    NEED(dr && dc && dwt && dta);
    TRY(score_bwd(U, B, dlogit, dr, dc, st, ce));
    // dwt = dr W_a^T + dc (x) b_a,  dta = dwt * w_out: one launch (rank-1 term and column scale in
    // the epilogue of the product) where the short-reduction kernel covers the shape
    bool dta_done = false;
    {
        Seg sg{dr, F, w->w_a, F, F};
        LinearOut o{};
        o.y = dta; o.ldy = D; o.y_pre = dwt; o.ldy_pre = D; o.epi = EPI_MUL; o.mul = w->w_out;
        o.r1_s = dc; o.r1_v = w->b_a;
        const int rc = linear_nt(&sg, 1, B, D, o, ar.rest(), ar.rest_n(), st);
        if (rc == SF_OK) dta_done = true;
        else if (rc != SF_ERR_UNSUPPORTED) return rc;
    }
    if (!dta_done) {
        TRY(linear_plain(dr, F, w->w_a, F, nullptr, B, D, F, EPI_NONE, dwt, D, ar, st));
        TRY(rank1_add(dc, w->b_a, B, D, dwt, D, st));
    }
    if (g) {
        if (g->w_a) TRY(gemm_tn(wt, D, dr, F, B, D, F, g->w_a, F, 1, st, ar.rest(), ar.rest_n()));
        if (g->b_a) TRY(dot_rows_accum(dc, wt, D, B, D, g->b_a, st));
        if (g->b_out) TRY(sum_accum(dc, B, g->b_out, st));
        if (g->w_out) TRY(colsum_prod(dwt, D, t_a, D, B, D, g->w_out, st));
    }
    if (!dta_done) TRY(scale_cols(dwt, D, w->w_out, B, D, dta, D, st));
    if (dh && tanh_of && w->w_h_t) {
        // dh <- (dta W_h) * (1 - tanh_of^2): the backward through h~ = tanh(.) rides in the epilogue
        Seg sg{dta, D, w->w_h_t, D, D};
        LinearOut o{};
        o.y = dh; o.ldy = H; o.epi = EPI_TANHBWD; o.aux = tanh_of; o.ld_aux = H;
        const int rc = linear_nt(&sg, 1, B, H, o, ar.rest(), ar.rest_n(), st);
        if (rc == SF_OK) { if (tanh_done) *tanh_done = true; }
        else if (rc != SF_ERR_UNSUPPORTED) return rc;
        else TRY(data_grad(dta, D, w->w_h, w->w_h_t, B, D, H, dh, H, 0, ar, st));
    } else if (dh) {
        TRY(data_grad(dta, D, w->w_h, w->w_h_t, B, D, H, dh, H, 0, ar, st));
    }
    if (g && g->w_h) TRY(gemm_tn(dta, D, h, H, B, D, H, g->w_h, H, 1, st, ar.rest(), ar.rest_n()));
    if (g && g->b_h) TRY(colsum(dta, D, B, D, g->b_h, 1, st, nullptr, ar.rest(), ar.rest_n()));
    return SF_OK;
}

}  // namespace sf

using namespace sf;

extern "C" {

size_t sf_workspace_bytes(void) { return WORKSPACE_BYTES; }
size_t sf_wgrad_workspace_bytes(void) { return WGRAD_WORKSPACE_BYTES; }
int sf_abi_version(void) { return SF_ABI_VERSION; }
#ifndef SF_BUILD_ID
#define SF_BUILD_ID "unknown"
#endif
// (the marker in front of the id lets build.py read it from the file without loading the library)
const char* sf_build_id(void) { static const char id[] = "SF_BUILD_ID=" SF_BUILD_ID; return id + 12; }
void sf_debug_persist_timeout(long long ticks) { sf::g_persist_timeout = ticks; }
void sf_debug_gate_product_f32(int on) { sf::g_nt_force_f32 = on; }
void sf_debug_many_row_product(int on) { sf::g_nt_big = on & 1; sf::g_nt_big_ksplit = (on & 2) ? 0 : 1; }
void sf_debug_grouped_weight_gradients(int on) { sf::g_tn_group = on; }
void sf_debug_slab_consumers(int on) { g_slab_consumers = on; }
int sf_debug_cotenant(int blocks, int threads, int lds_bytes, long long ticks, float* sink, sf_stream stream) {
    SF_ENTER();
    return sf::cotenant(blocks, threads, lds_bytes, ticks, sink, S(stream));
}
void sf_gate_product_strict(int on) { sf::g_nt_force_f32 = on ? 1 : 0; }
int sf_gate_product_is_strict(void) { return sf::g_nt_force_f32 != 0; }
void sf_debug_projected_partials_late(int on) { g_proj_partials_late = on; }
void sf_debug_projected_text_groups(int groups) { sf::g_proj_text_groups = groups == 2 || groups == 4 ? groups : 0; }
int sf_debug_projected_attention(const sf_pano* X, int B, int H, const float* pv, const float* lv, int ld, const float* h1,
                                 int ldh1, float* alpha, float* out, int ldo, int late, void* ws, size_t ws_bytes,
                                 sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(X && pv && lv && h1 && alpha && out && B > 0 && H > 0);
    const PanoSrc x = pano(X);
    Arena ar = arena(ws, ws_bytes);
    float* part = ar.take(visual_attn_split_floats(B, x.IMG + x.LOC));
    if (!part || !ar.tickets()) return SF_ERR_WORKSPACE;
    return proj_attention_alone(x, B, ProjTables{pv, nullptr, lv, nullptr, ld, H}, h1, ldh1, alpha, out, ldo, late, part,
                                ar.tickets(), S(stream));
}
void sf_debug_precise_attention(int on) { sf::g_precise_attention = on; }
void sf_debug_tn_split_min_rows(int rows) { sf::g_tn_split_min_rows = rows < 0 ? 4096 : rows; }
size_t sf_workspace_fault_offset(size_t ws_bytes) {
    const size_t n = ws_bytes / 4;
    if (n <= SYNC_WORDS) return 0;
    return (n - SYNC_WORDS + PERSIST_TICKET + persistent_fault_word()) * 4;
}
const char* sf_last_error_string(void) { return hipGetErrorString(g_last_hip_error); }
const char* sf_status_string(int s) {
    switch (s) {
        case SF_OK: return "ok";
        case SF_ERR_ARG: return "invalid argument";
        case SF_ERR_UNSUPPORTED: return "unsupported shape";
        case SF_ERR_LAUNCH: return "kernel launch failed";
        case SF_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown status";
    }
}

int sf_linear_fwd(const float* x, int ldx, const float* w, const float* b, int M, int N, int K,
                  int act, float* y, int ldy, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(x && w && y && M > 0 && N > 0 && K > 0 && (act == 0 || act == 1));
    return linear_plain(x, ldx, w, K, b, M, N, K, act ? EPI_TANH : EPI_NONE, y, ldy,
                        arena(ws, ws_bytes), S(stream));
}

int sf_linear_slabs_fwd(const float* x, int ldx, const float* w, int K1, const float* h, int ldh,
                        const float* u, int K2, int M, int N, int* ksplit, void* ws, size_t ws_bytes,
                        sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(x && w && ksplit && ws && M > 0 && N > 0 && K1 > 0 && (!h || (u && K2 > 0)));
    Arena ar = arena(ws, ws_bytes);
    Seg segs[2] = {{x, ldx, w, K1, K1}, {h, ldh, u, K2, K2}};
    LinearOut o{};
    float* slabs = nullptr;
    const void* packed[2];
    const bool bf16w = bf16_packed(w, h ? u : nullptr, packed);
    return linear_nt(segs, h ? 2 : 1, M, N, o, ar.rest(), ar.rest_n(), S(stream), &slabs, ksplit, bf16w ? packed : nullptr);
}

int sf_linear_bwd(const float* x, int ldx, const float* w, const float* y, int ldy, const float* dy,
                  int lddy, int M, int N, int K, int act, float* dx, int lddx, int accumulate_dx,
                  float* dw, float* db, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(x && w && dy && M > 0 && N > 0 && K > 0 && (N % 4 == 0) && (K % 4 == 0));
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    const float* dpre = dy;
    int ldp = lddy;
    if (act == 1) {
        SF_CHECK_ARG(y);
        float* t = ar.take((size_t)M * N);
        NEED(t);
        TRY(tanh_bwd(y, ldy, dy, lddy, M, N, t, N, st));
        dpre = t;
        ldp = N;
    }
    if (dx) TRY(gemm_nn_ws(dpre, ldp, w, K, M, K, N, dx, lddx, accumulate_dx, ar.rest(), ar.rest_n(), st));
    if (dw) TRY(gemm_tn(dpre, ldp, x, ldx, M, N, K, dw, K, 1, st, ar.rest(), ar.rest_n()));
    if (db) TRY(colsum(dpre, ldp, M, N, db, 1, st, nullptr, ar.rest(), ar.rest_n()));
    return SF_OK;
}

int sf_lstm_cell_fwd(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx,
                     const float* h0, const float* c0, float* h1, float* c1, float* gates,
                     float* h1_drop, int ld_h1_drop, const sf_dropout* drop, uint32_t drop_stream,
                     void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && x && h0 && c0 && h1 && c1 && B > 0 && I > 0 && H > 0 && H % 4 == 0);
    return lstm_fwd_i(w, B, I, H, x, ldx, h0, c0, h1, c1, gates, h1_drop, ld_h1_drop,
                      make_dropout(drop, drop_stream), arena(ws, ws_bytes), S(stream));
}

int sf_lstm_cell_rows_fwd(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx, int x_col0, const float* xg,
                          const float* xg2, const float* h0, const float* c0, float* h1, float* c1, float* gates, int path,
                          void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && x && xg && h0 && c0 && h1 && c1 && B > 0 && H > 0 && H % 4 == 0 && x_col0 > 0 && x_col0 < I &&
                 x_col0 % 4 == 0 && I % 4 == 0 && ldx % 4 == 0 && path >= 0 && path <= 2);
    return lstm_fwd_i(w, B, I, H, x, ldx, h0, c0, h1, c1, gates, nullptr, 0, Dropout{}, arena(ws, ws_bytes), S(stream), xg,
                      x_col0, xg2, path);
}

int sf_lstm_cell_rows3_fwd(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx, int x_col0, const float* xg,
                           const float* xg2, const float* xg_h, const float* h0, const float* c0, float* h1, float* c1,
                           float* gates, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && x && xg && xg2 && xg_h && h0 && c0 && h1 && c1 && B > 0 && H > 0 && H % 4 == 0 && x_col0 > 0 &&
                 x_col0 < I && x_col0 % 4 == 0 && I % 4 == 0 && ldx % 4 == 0);
    return lstm_fwd_i(w, B, I, H, x, ldx, h0, c0, h1, c1, gates, nullptr, 0, Dropout{}, arena(ws, ws_bytes), S(stream), xg,
                      x_col0, xg2, 0, xg_h);
}

int sf_debug_recurrent_row(const sf_lstm_w* w, int B, int H, const float* h1, int ldh1, float* xg_h, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && w->w_hh && w->b_ih && w->b_hh && h1 && xg_h && B > 0 && H > 0 && H % 4 == 0 && ldh1 % 4 == 0 && ldh1 >= H);
    Seg sg{h1, ldh1, w->w_hh, H, H};
    LinearOut o{};
    o.y = xg_h; o.ldy = 4 * H; o.bias = w->b_ih; o.bias2 = w->b_hh; o.epi = EPI_NONE;
    SmallPlan p;
    if (!linear_small_plan(&sg, 1, B, 4 * H, o, &p)) return SF_ERR_UNSUPPORTED;
    return proj_score_hh_alone(p, S(stream));
}

int sf_lstm_cell_bwd(const sf_lstm_w* w, const sf_lstm_g* g, int B, int I, int H, const float* x,
                     int ldx, const float* h0, const float* c0, const float* c1, const float* gates,
                     const float* dh1, const float* dc1, float* dx, int lddx, float* dh0, float* dc0,
                     void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && x && h0 && c0 && c1 && gates && dc0 && B > 0 && H % 4 == 0 && I % 4 == 0);
    return lstm_bwd_i(w, g, B, I, H, x, ldx, h0, c0, c1, gates, dh1, nullptr, dc1, dx, lddx, dh0,
                      dc0, arena(ws, ws_bytes), S(stream));
}

int sf_visual_attention_fwd(const sf_visual_w* w, const sf_pano* X, int B, int H, int D,
                            const float* h, float* out, int ldo, float* alpha, float* t_v, float* q,
                            const sf_dropout* drop, uint32_t drop_stream, int drop_col0, void* ws,
                            size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && X && h && out && alpha && t_v && q && B > 0);
    return visual_fwd_i(w, pano(X), B, H, D, h, out, ldo, alpha, t_v, q,
                        make_dropout(drop, drop_stream), drop_col0, arena(ws, ws_bytes), S(stream));
}

int sf_visual_attention_fwd_f64(const sf_visual_w* w, const sf_pano* X, int B, int H, int D,
                                const float* h, float* out, int ldo, float* alpha, float* t_v, float* q,
                                const sf_dropout* drop, uint32_t drop_stream, int drop_col0, void* ws,
                                size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && X && h && out && alpha && t_v && q && B > 0);
    const PanoSrc src = pano(X);
    const int F = src.IMG + src.LOC;
    Arena ar = arena(ws, ws_bytes);
    if (!w->w_v_t || !visual_attn_f64_supported(src, B) || (H & 3) || (D & 3) || !ar.tickets() ||
        ar.rest_n() < (size_t)B * (D + F) * 2 + visual_attn_split_floats(B, F) + 256)
        return SF_ERR_UNSUPPORTED;
    return visual_fwd_i(w, src, B, H, D, h, out, ldo, alpha, t_v, q, make_dropout(drop, drop_stream), drop_col0, ar,
                        S(stream), true);
}

int sf_linear_f64(const float* x, int ldx, const float* w, int ldw, const float* b, int M, int N, int K, double* y64,
                  float* y32, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(x && w && (y64 || y32) && M > 0 && N > 0 && K > 0);
    return linear_f64(x, nullptr, ldx, w, ldw, b, M, N, K, y64, N, y32, N, S(stream));
}

int sf_visual_attention_bwd(const sf_visual_w* w, const sf_visual_g* g, const sf_pano* X, int B,
                            int H, int D, const float* h, const float* alpha, const float* t_v,
                            const float* dout, int lddo, const sf_dropout* drop,
                            uint32_t drop_stream, int drop_col0, float* dh, void* ws,
                            size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && X && h && alpha && t_v && dout && B > 0);
    return visual_bwd_i(w, g, pano(X), B, H, D, h, alpha, t_v, dout, lddo,
                        make_dropout(drop, drop_stream), drop_col0, dh, arena(ws, ws_bytes),
                        S(stream));
}

int sf_visual_query_fold_f64(const sf_visual_w* w, int H, int D, int F, double* m_v, double* c_v, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && w->w_v_t && w->w_h_t && w->b_h && m_v && c_v && H > 0 && D > 0 && F > 0 && !(D & 3));
    // M_v[F,H] = W_v^T[F,D] (W_h^T[H,D])^T, c_v[1,F] = b_h[1,D] (W_v^T[F,D])^T -- both accumulated and kept in float64
    TRY(linear_f64(w->w_v_t, nullptr, D, w->w_h_t, D, nullptr, F, H, D, m_v, H, nullptr, 0, S(stream)));
    return linear_f64(w->b_h, nullptr, D, w->w_v_t, D, nullptr, 1, F, D, c_v, F, nullptr, 0, S(stream));
}

int sf_soft_dot_attention_fwd(const sf_softdot_w* w, int B, int L, int H, const float* h, int ldh,
                              const float* ctx, const uint8_t* mask, const int32_t* ctx_row,
                              float* h_tilde, float* alpha, float* cat2, float* t_text, void* ws,
                              size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && h && ctx && h_tilde && alpha && cat2 && t_text && B > 0 && L > 0);
    return softdot_fwd_i(w, B, L, H, h, ldh, ctx, mask, h_tilde, alpha, cat2, t_text,
                         arena(ws, ws_bytes), S(stream), ctx_row);
}

int sf_soft_dot_attention_bwd(const sf_softdot_w* w, const sf_softdot_g* g, int B, int L, int H,
                              const float* ctx, const float* alpha, const float* cat2,
                              const float* t_text, const float* h_tilde, const float* dh_tilde,
                              float* dh, int lddh, float* dctx, void* ws, size_t ws_bytes,
                              sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && ctx && alpha && cat2 && t_text && h_tilde && dh_tilde && dh && B > 0);
    return softdot_bwd_i(w, g, B, L, H, ctx, alpha, cat2, t_text, h_tilde, dh_tilde, dh, lddh, dctx,
                         arena(ws, ws_bytes), S(stream));
}

// ContextOnlySoftDotAttention core (model.py:166-177 behind its linear_in): scores, masked softmax, weighted context
int sf_text_attention_fwd(const float* ctx, const uint8_t* mask, int B, int L, int H, const float* t, int ldt,
                          float* alpha, float* wc, int ldwc, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(ctx && t && alpha && wc && B > 0 && L > 0 && H > 0);
    return text_attn_fwd(ctx, mask, B, L, H, t, ldt, alpha, wc, ldwc, S(stream));
}

int sf_text_attention_bwd(const float* ctx, int B, int L, int H, const float* dwc, int lddwc, const float* t, int ldt,
                          const float* alpha, float* dt, int lddt, float* dctx, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(ctx && dwc && t && alpha && dt && B > 0 && L > 0 && H > 0);
    return text_attn_bwd(ctx, B, L, H, dwc, lddwc, t, ldt, alpha, dt, lddt, dctx, S(stream));
}

int sf_eltwise_prod_scoring_fwd(const sf_scoring_w* w, const sf_cands* U, int B, int H, int D,
                                const float* h, float* logit, float* t_a, float* wt, float* r,
                                void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && U && h && logit && t_a && wt && r && B > 0);
    return scoring_fwd_i(w, cands(U), B, H, D, h, logit, t_a, wt, r, arena(ws, ws_bytes), S(stream));
}

int sf_eltwise_prod_scoring_bwd(const sf_scoring_w* w, const sf_scoring_g* g, const sf_cands* U,
                                int B, int H, int D, const float* h, const float* t_a,
                                const float* wt, const float* dlogit, float* dh, void* ws,
                                size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && U && h && t_a && wt && dlogit && B > 0);
    return scoring_bwd_i(w, g, cands(U), B, H, D, h, t_a, wt, dlogit, dh, arena(ws, ws_bytes),
                         S(stream));
}

// ---- a11 gathers ---------------------------------------------------------------------------------------
int sf_gather_panorama(const sf_pano* X, int B, float* out, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(X && out && B > 0 && X->table && X->loc_table && X->vp && X->view);
    return gather_panorama(pano(X), B, out, S(stream));
}
int sf_gather_candidates(const sf_cands* U, int B, float* all_u, float* is_valid, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(U && all_u && B > 0 && U->table && U->vp && U->cand_view && U->cand_sincos && U->a_num);
    return gather_candidates(cands(U), B, all_u, is_valid, S(stream));
}
int sf_gather_actions(const sf_cands* U, int B, const int32_t* a, float* out, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(U && a && out && B > 0 && U->table && U->vp && U->cand_view && U->cand_sincos && U->a_num);
    return gather_actions(cands(U), B, a, out, S(stream));
}

int sf_gather_actions_ld(const sf_cands* U, int B, const int32_t* a, float* out, int ld_out, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(U && a && out && B > 0 && ld_out > 0 && U->table && U->vp && U->cand_view && U->cand_sincos && U->a_num);
    return gather_actions(cands(U), B, a, out, S(stream), ld_out);
}

int sf_gather_path_actions(const float* table, int V, int IMG, int LOC, const int32_t* vp, const int32_t* act_view,
                           const float* act_sincos, const int32_t* act, int N, float* out, int ld_out,
                           sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(table && vp && act_view && act_sincos && act && out && N > 0 && V > 0 && ld_out >= IMG + LOC);
    return gather_path_actions(table, V, IMG, LOC, vp, act_view, act_sincos, act, N, out, ld_out, S(stream),
                               table_is_f16(table));
}

// ---- search helpers -----------------------------------------------------------------------
int sf_gather_rows(const float* src, int ld_src, const int32_t* idx, int n, int width, float* dst,
                   int ld_dst, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(src && idx && dst && n > 0 && width > 0);
    return gather_rows(src, ld_src, idx, n, width, dst, ld_dst, S(stream));
}

int sf_logprob_topk(float* logit, int ld, int N, int n, const int32_t* n_valid, int k, int32_t* idx,
                    float* logp, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(logit && logp && N > 0 && n > 0 && ld >= n && (idx || k == n));
    return logprob_topk(logit, ld, N, n, n_valid, k, idx, logp, S(stream));
}
int sf_scatter_rows(const float* src, int ld_src, const int32_t* idx, int n, int width, float* dst,
                    int ld_dst, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(src && idx && dst && n > 0 && width > 0);
    return scatter_rows(src, ld_src, idx, n, width, dst, ld_dst, S(stream));
}
int sf_speaker_beam_select(const sf_spk_beam* s, const int32_t* top_w, const float* top_lp, const float* alpha,
                           sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(s && top_w && top_lp && s->B > 0 && s->beam_size > 0 && s->k >= 1 && s->k <= s->beam_size &&
                 s->T > 0 && s->Tp > 0 && s->eos >= 0);
    SF_CHECK_ARG(s->score && s->words && s->parent && s->inst && s->live_total && s->hist_word && s->hist_parent &&
                 s->hist_score && s->done_rec && s->done_score && !s->hist_attn == !alpha);
    const int64_t R = (int64_t)s->B * s->beam_size;
    SF_CHECK_ARG(s->ld_hist >= R && (!s->hist_attn || s->ld_hist >= R * s->Tp));
    return speaker_beam_select(*s, top_w, top_lp, alpha, S(stream));
}
int sf_follower_beam_select(const sf_fol_beam* s, const int32_t* top_a, const float* top_lp, const float* alpha,
                            sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(s && top_a && top_lp && s->B > 0 && s->beam_size > 0 && s->k >= 1 && s->k <= s->beam_size &&
                 s->episode_len > 0 && s->T > 0);
    SF_CHECK_ARG(s->nav.a_num && s->nav.next_row && s->nav.cand_view && s->nav.A > 0 && s->nav.V > 0 &&
                 s->k <= s->nav.A);
    SF_CHECK_ARG(s->score && s->row && s->view && s->act && s->parent && s->inst && s->live_total && s->hist_parent &&
                 s->hist_action && s->hist_rank && s->hist_sid && s->hist_psid && s->hist_score && s->done_rec &&
                 s->done_score && !s->hist_attn == !alpha);
    const int64_t R = (int64_t)s->B * s->beam_size;
    SF_CHECK_ARG(s->ld_hist >= R && (!s->hist_attn || s->ld_hist >= R * s->T));
    return follower_beam_select(*s, top_a, top_lp, alpha, S(stream));
}
int sf_state_factored_select(const sf_state_search* s, const float* logp, int ld_logp, int32_t* dev_in,
                             sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(s && logp && dev_in);
    SF_CHECK_ARG(s->B > 0 && s->successor_size > 0 && s->completion_size > 0 && s->episode_len > 0 &&
                 s->key_fields >= 1 && s->key_fields <= 4 && s->n_keys > 0 && s->node_cap > 0 && s->slot_cap > 0 &&
                 s->visit_cap > 0 && s->pool_rows > 0);
    SF_CHECK_ARG(s->nav.a_num && s->nav.next_row && s->nav.cand_view && s->nav.A > 0 && s->nav.V > 0 &&
                 ld_logp >= s->nav.A);
    SF_CHECK_ARG((int64_t)s->cap >= (int64_t)s->B * s->successor_size &&
                 (int64_t)s->B * s->node_cap < ((int64_t)1 << 31) && (int64_t)s->B * s->n_keys < ((int64_t)1 << 40));
    SF_CHECK_ARG(s->base_row && s->status && s->inst && s->frontier && s->node_parent && s->node_sid && s->node_key &&
                 s->node_action && s->node_count && s->node_pool && s->node_start && s->node_born && s->node_score &&
                 s->open_slot && s->open_key && s->open_node && s->open_pick && s->held_slot && s->held_key &&
                 s->held_node && s->held_pick && s->comp_node && s->comp_order && s->visits);
    return state_factored_select(*s, logp, ld_logp, dev_in, S(stream));
}

// ---- movers, optimizer, small copies ----------------------------------------------------------------------
int sf_fill_f32(float* p, size_t n, float v, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(p || n == 0);
    return fill(p, n, v, S(stream));
}

int sf_move_rows(const sf_row_move* moves, int n_moves, int n, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(moves && n_moves >= 1 && n_moves <= SF_ROW_MOVES_MAX && n >= 0);
    if (n == 0) return SF_OK;
    RowMoves mv;
    mv.n = n_moves;
    for (int i = 0; i < n_moves; ++i) {
        const sf_row_move& m = moves[i];
        SF_CHECK_ARG(m.src && m.dst && m.idx && m.width > 0 && m.ld_src >= m.width && m.ld_dst >= m.width);
        mv.m[i] = RowMoves::M{m.src, m.dst, m.idx, m.ld_src, m.ld_dst, m.width, m.scatter ? 1 : 0};
    }
    return move_rows(mv, n, S(stream));
}

int sf_fill_regions(const sf_fill_region* regions, int n, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(n >= 0 && n <= SF_FILL_MAX_REGIONS && (regions || n == 0));
    FillRegions fr;
    fr.n = 0;
    for (int i = 0; i < n; ++i) {
        const sf_fill_region& r = regions[i];
        SF_CHECK_ARG(r.width == 1 || r.width == 4 || r.width == 8);
        SF_CHECK_ARG(r.ptr || r.count == 0);
        SF_CHECK_ARG(((uintptr_t)r.ptr & (uintptr_t)(r.width - 1)) == 0);
        if (r.count == 0) continue;
        fr.r[fr.n++] = FillRegions::R{r.ptr, (unsigned long long)r.count, (unsigned long long)r.value, r.width};
    }
    if (fr.n == 0) return SF_OK;
    return fill_regions(fr, S(stream));
}

int sf_add_f32(float* dst, const float* src, size_t n, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG((dst && src) || n == 0);
    if (n == 0) return SF_OK;
    if (n > (size_t)INT_MAX) return SF_ERR_UNSUPPORTED;       // add2 takes its width as an int
    return add2(dst, 0, src, 0, 1, (int)n, dst, 0, S(stream));
}

int sf_adam_step(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int step, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG((p && g && m && v) || n == 0);
    SF_CHECK_ARG(step >= 1 && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1.);
    if (n == 0) return SF_OK;
    return adam_step(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, S(stream));
}

int sf_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1, double beta2,
                     double eps, double weight_decay, int32_t* step_dev, float* coef, const uint32_t* skip_if_nonzero, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(((p && g && m && v) || n == 0) && step_dev && coef);
    SF_CHECK_ARG(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1.);
    return adam_step_dev(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step_dev, coef, skip_if_nonzero, S(stream));
}

int sf_store_u32x4(uint32_t* dst, uint32_t a, uint32_t b, uint32_t c, uint32_t d, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(dst != nullptr);
    return store_u32x4(dst, a, b, c, d, S(stream));
}

int sf_site_advance(uint32_t* word, uint32_t by, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(word != nullptr);
    return site_advance(word, by, S(stream));
}

int sf_dropout_copy(const float* src, int lds, int B, int N, float* dst, int ldd,
                    const sf_dropout* drop, uint32_t drop_stream, int col0, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(src && dst && B > 0 && N > 0);
    return dropout_copy(src, lds, B, N, dst, ldd, make_dropout(drop, drop_stream), col0, S(stream));
}

int sf_transpose(const float* src, int R, int Ccols, float* dst, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(src && dst && R > 0 && Ccols > 0);
    return transpose(src, R, Ccols, dst, S(stream));
}

int sf_embedding_fwd(const float* table, int E, const int64_t* idx, int B, float* out,
                     sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(table && idx && out && B > 0 && E > 0);
    return embedding_rows(table, E, idx, B, out, S(stream));
}

// ---- in-process kernel timing ---------------------------------------------------------------------
int sf_profile_begin(void) {
    SF_ENTER();
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    if (g_prof.active) return SF_ERR_ARG;
    g_prof.recs.clear();
    g_prof.used = 0;
    g_prof.active = true;
    return SF_OK;
}

long sf_profile_end(char* buf, size_t cap) {
    SF_ENTER();
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    if (!g_prof.active) return -1;
    g_prof.active = false;
    struct Row { long calls = 0; double total = 0, mn = 1e30, mx = 0; };
    std::map<std::string, Row> rows;
    for (const ProfRec& r : g_prof.recs) {
        if (!r.e0 || !r.e1) return -1;
        if (hipEventSynchronize(r.e1) != hipSuccess) return -1;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) return -1;
        Row& w = rows[r.name];
        const double us = 1e3 * (double)ms;
        w.calls += 1; w.total += us; w.mn = std::min(w.mn, us); w.mx = std::max(w.mx, us);
    }
    g_prof.recs.clear();
    g_prof.used = 0;
    std::string out;
    char line[512];
    for (const auto& kv : rows) {
        snprintf(line, sizeof line, "%s\t%ld\t%.3f\t%.3f\t%.3f\n", kv.first.c_str(), kv.second.calls,
                 kv.second.total, kv.second.mn, kv.second.mx);
        out += line;
    }
    if (buf && cap) {
        const size_t n = std::min(cap - 1, out.size());
        std::copy(out.begin(), out.begin() + (long)n, buf);
        buf[n] = 0;
    }
    return (long)out.size() + 1;
}

}  // extern "C"
