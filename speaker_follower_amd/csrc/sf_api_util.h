// What the translation units of the C entry layer (sf_api*.hip) share: the workspace arena, the status macros, the
// C-struct -> kernel-source conversions, the address registry, and the declarations of the composite helpers and
// globals that more than one unit uses.  Host-only: no kernel, nothing mutable.
#pragma once
#include "sf_kernels.h"
#include "sf_gemm_small.h"
#include "sf_glue.h"

#include <atomic>
#include <mutex>

namespace sf {

// Bump allocator over the caller's workspace.  Passed BY VALUE into helpers so that their
// temporaries are released on return; whatever is left is handed to the GEMMs for split-K slabs.
struct Arena {
    float* base;
    size_t cap, off;
    unsigned* tk = nullptr;   // the workspace's ticket region (set by arena(); sub-arenas carry it along)
    float* take(size_t n) {
        n = (n + 63) & ~(size_t)63;
        if (off + n > cap) return nullptr;
        float* p = base + off;
        off += n;
        return p;
    }
    float* rest() const { return base + off; }
    size_t rest_n() const { return cap - off; }
    // the last SYNC_WORDS dwords of the workspace: monotonic ticket counters (zero-initialised by
    // the caller once, see sf_workspace_bytes); never handed out by take()
    unsigned* tickets() const { return tk; }
};
constexpr size_t SYNC_WORDS = 2048;        // [0, 1024): per-sample tickets of the split attention kernels
constexpr size_t PERSIST_TICKET = 1100;   // [1100, 1140): arrival counter + placement record of the persistent launches
constexpr size_t TEXT_TICKET = 1200;      // [1200, 1712): per-sample tickets of the folded text attention (B <= 512)

inline Arena arena(void* ws, size_t bytes) {
    const size_t n = ws ? bytes / 4 : 0;
    const size_t usable = n > SYNC_WORDS ? n - SYNC_WORDS : 0;
    return Arena{(float*)ws, usable, 0, usable ? reinterpret_cast<unsigned*>((float*)ws + usable) : nullptr};
}
inline hipStream_t S(sf_stream s) { return (hipStream_t)s; }

#define TRY(expr)                     \
    do {                              \
        int _st = (expr);             \
        if (_st != SF_OK) return _st; \
    } while (0)
#define NEED(ptr) \
    if (!(ptr)) return SF_ERR_WORKSPACE

template <class T>
inline T* adv(T* p, size_t n) { return p ? p + n : nullptr; }

// ---- address registry ---------------------------------------------------------------------------------------------------
// The C structs carry no tag for what the library knows about a buffer (their layout is pinned by the ABI): a feature
// table is known to hold binary16, or to have projected tables / gate-space rows, and an LSTM's weights to have packed
// bf16 images, by ADDRESS.  CAP entries behind the registry's own mutex; the same key replaces in place, forgetting an
// unknown key is fine, and a key beyond CAP is SF_ERR_UNSUPPORTED until one is forgotten.
template <class Key, class Value, int CAP = 16>
class Registry {
    struct Slot { Key key; Value value; };
    Slot slot_[CAP];
    int n_ = 0;
    mutable std::mutex mutex_;
    int at(const Key& key) const {
        for (int i = 0; i < n_; ++i)
            if (slot_[i].key == key) return i;
        return -1;
    }

public:
    int put(const Key& key, const Value& value) {
        std::lock_guard<std::mutex> lock(mutex_);
        int i = at(key);
        if (i < 0) {
            if (n_ == CAP) return SF_ERR_UNSUPPORTED;
            i = n_++;
        }
        slot_[i] = Slot{key, value};
        return SF_OK;
    }
    int forget(const Key& key) {
        std::lock_guard<std::mutex> lock(mutex_);
        const int i = at(key);
        if (i >= 0) slot_[i] = slot_[--n_];
        return SF_OK;
    }
    bool find(const Key& key, Value* out) const {
        std::lock_guard<std::mutex> lock(mutex_);
        const int i = at(key);
        if (i < 0) return false;
        if (out) *out = slot_[i].value;
        return true;
    }
};

// ---- the registries' lookups (sf_api_tables.hip) ------------------------------------------------------------------------
int table_is_f16(const void* table);                               // sf_feature_table_f16
bool projected_lookup(const void* table, sf_projected* out);       // sf_projected_register, where sf_projected_use is on
bool gate_rows_lookup(const void* table, sf_gate_rows* out);       // sf_gate_rows_register, where sf_gate_rows_use is on
bool gate_rows_attended_lookup(const void* table, sf_gate_rows_attended* out);   // ... _attended_register / _attended_use
// the packed images of (w_ih, w_hh) when the switch is on and the pair is registered; false: today's kernels
bool bf16_packed(const float* w_ih, const float* w_hh, const void* (&packed)[2]);
inline int projected_ld(int H) { return (H + 1 + 3) & ~3; }
extern std::atomic<long long> g_proj_steps;     // sf_projected_steps: decode steps issued on the projected chain
extern std::atomic<long long> g_gate_steps;     // sf_gate_rows_steps: decode steps whose gate product ran on a gate-space row
extern std::atomic<long long> g_gate_att_steps; // sf_gate_rows_attended_steps: ... whose cell added an attended row too
extern std::atomic<long long> g_gate_rec_steps; // sf_gate_rows_recurrent_steps: ... whose cell added the recurrent row too
bool gate_rows_recurrent_on();                  // sf_gate_rows_recurrent_use (sf_api_tables.hip)
extern int g_proj_partials_late;                // sf_debug_projected_partials_late (sf_api.hip)

// the ONLY places that turn the C structs into the kernels' sources: a dense source is never half
inline PanoSrc pano(const sf_pano* p) {
    return PanoSrc{p->dense, p->table, p->loc_table, p->vp, p->view, p->V, p->IMG, p->LOC,
                   p->dense ? 0 : table_is_f16(p->table)};
}
inline CandSrc cands(const sf_cands* c) {
    return CandSrc{c->dense, c->table, c->vp, c->cand_view, c->cand_sincos, c->a_num,
                   c->A, c->V, c->IMG, c->LOC, c->dense ? 0 : table_is_f16(c->table)};
}

inline FGlue make_glue(const CandSrc& src, int B, float* logit, const sf_follower_glue* g) {
    FGlue f{};
    f.src = src; f.B = B; f.logit = logit; f.is_valid = g->is_valid; f.target = g->target;
    f.feedback = g->feedback; f.ended = g->ended; f.a_t = g->a_t; f.target_used = g->target_used;
    f.score = g->score; f.u_next = g->u_next; f.ld_u = g->ld_u_next;
    f.u_drop = make_dropout(g->u_drop, g->u_drop_stream, 2);     // (numbered 2 * (step + 1))
    f.ce_term = g->ce_term; f.live = g->live; f.sample_seed = g->sample_seed;
    f.sample_stream = g->sample_stream; f.row0 = g->row0;
    f.sample_site = g->sample_site_dev ? g->sample_site_dev : site_zero();
    if (g->nav) {
        const sf_nav_io& n = *g->nav;
        f.nav = NavIO{n.nav, n.row, n.view, n.goal_hop, n.ld_hop, n.hop_base, n.row_next, n.vp_next, n.view_next,
                      n.a_num_next, n.cand_view_next, n.sincos_next, n.target_next, true};
    }
    return f;
}
inline bool glue_ok(const sf_cands* U, const sf_follower_glue* g) {
    return g->target && g->ended && g->a_t && g->target_used && g->score && g->ce_term && g->live &&
           g->feedback >= 0 && g->feedback <= 2 && (g->is_valid || U->a_num) &&
           (!g->u_next || g->ld_u_next % 4 == 0) &&
           (!g->nav || (g->nav->nav.A == U->A && g->nav->nav.a_num && g->nav->nav.next_row && g->nav->nav.cand_view &&
                        g->nav->nav.cand_sincos && g->nav->nav.feat_row && g->nav->row && g->nav->view &&
                        g->nav->row_next && g->nav->vp_next && g->nav->view_next && g->nav->a_num_next &&
                        g->nav->cand_view_next && g->nav->sincos_next &&
                        (!g->nav->target_next || (g->nav->goal_hop && g->nav->hop_base && g->nav->ld_hop > 0))));
}

// b_ih and b_hh of an LSTM have the same gradient (the column sums of dgates): one pass, two outputs
inline int colsum_pair(const float* Y, int ldy, int M, int N, float* a, float* b, Arena ar, hipStream_t st) {
    float* first = a ? a : b;
    if (!first) return SF_OK;
    return colsum(Y, ldy, M, N, first, 1, st, (a && b) ? b : nullptr, ar.rest(), ar.rest_n());
}

inline int linear_plain(const float* x, int ldx, const float* w, int ldw, const float* b, int M, int N,
                        int K, Epi epi, float* y, int ldy, Arena ar, hipStream_t st) {
    Seg sg{x, ldx, w, ldw, K};
    LinearOut o{};
    o.y = y;
    o.ldy = ldy;
    o.bias = b;
    o.epi = epi;
    return linear_nt(&sg, 1, M, N, o, ar.rest(), ar.rest_n(), st);
}

// dx[M,K] (+)= dy[M,N] * W[N,K].  With W^T ([K,N]) at hand this is a K-contiguous NT product.
inline int data_grad(const float* dy, int lddy, const float* w, const float* w_t, int M, int N, int K,
                     float* dx, int lddx, int accumulate, Arena ar, hipStream_t st) {
    if (w_t && N % 4 == 0) {
        Seg sg{dy, lddy, w_t, N, N};
        LinearOut o{};
        o.y = dx; o.ldy = lddx; o.epi = EPI_NONE; o.accumulate = accumulate;
        return linear_nt(&sg, 1, M, K, o, ar.rest(), ar.rest_n(), st);
    }
    return gemm_nn_ws(dy, lddy, w, K, M, K, N, dx, lddx, accumulate, ar.rest(), ar.rest_n(), st);
}

// The folded text attention's two products over a context [M, H] that is constant over an episode (the follower's
// instruction, the speaker's path): cq = ctx W_in (so that ctx_l . (W_in h) = cq_l . h) and co = ctx W_out[:, :H]^T.
inline int context_fold(const float* ctx, const float* w_in_t, const float* w_out, int M, int H, float* cq, float* co,
                        Arena ar, hipStream_t st) {
    TRY(linear_plain(ctx, H, w_in_t, H, nullptr, M, H, H, EPI_NONE, cq, H, ar, st));
    return linear_plain(ctx, H, w_out, 2 * H, nullptr, M, H, H, EPI_NONE, co, H, ar, st);
}

// ---- the composite operators a1 - a4 (sf_api.hip), as the follower, encoder and speaker sequences call them --------------
int lstm_fwd_i(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx, const float* h0,
               const float* c0, float* h1, float* c1, float* gates, float* h1_drop, int ld_h1_drop,
               const Dropout& drop, Arena ar, hipStream_t st,
               const float* xg = nullptr, int x_col0 = 0,      // xg [B, 4H]: x[:, :x_col0] W_ih[:, :x_col0]^T, formed elsewhere
                                                               // (the product then starts at column x_col0 of x and W_ih)
               const float* xg2 = nullptr,     // with xg: a second [B, 4H] row formed elsewhere, of further columns below x_col0
                                               // (the fused step only: SF_ERR_UNSUPPORTED where the product + cell kernel run)
               int path = 0,                   // with xg: 0 short_gate_fused decides; 1 the product + cell kernel; 2 the fused step
               const float* xg_h = nullptr);   // with xg and xg2 (path 0): h0 W_hh^T + b_ih + b_hh formed elsewhere -- the step is
                                               // lstm_step_rows over x[:, x_col0:] alone (recurrent_row_cell, sf_gemm_plan.h);
                                               // SF_ERR_UNSUPPORTED, nothing launched, where that rule or a row is missing
// Whether a step with a gate-space row runs what is left of its product, K = I - x_col0 + H, inside the fused step kernel
// (lstm_step_fused: one launch, the rows added ahead of the cell) instead of as a K-split product plus the cell kernel.
// A pure function of the shape; the rule of the step WITHOUT a row (lstm_fwd_i: I + H <= 1024) applied to what remains.
inline bool short_gate_fused(int K_x, int H) { return K_x > 0 && K_x + H <= 1024 && H % 16 == 0 && K_x % 4 == 0; }
// (the step with the recurrent half as a third row, K = I - x_col0 alone: recurrent_row_cell, sf_gemm_plan.h -- a header
//  the host tests compile)
int lstm_bwd_i(const sf_lstm_w* w, const sf_lstm_g* g, int B, int I, int H, const float* x, int ldx,
               const float* h0, const float* c0, const float* c1, const float* gates,
               const float* dh1, const float* dh1_b, const float* dc1, float* dx, int lddx,
               float* dh0, float* dc0, Arena ar, hipStream_t st, float* dgates_out = nullptr,
               int dx_col0 = 0,            // dx is only formed for input columns >= dx_col0
               const Dropout* dh1b_drop = nullptr,     // mask still to be applied to dh1_b
               SmallPlan* dh0_plan = nullptr, bool* dh0_deferred = nullptr,
               const float** dx_slabs = nullptr, int* dx_ks = nullptr);
int visual_fwd_i(const sf_visual_w* w, const PanoSrc& X, int B, int H, int D, const float* h,
                 float* out, int ldo, float* alpha, float* t_v, float* q, const Dropout& drop,
                 int col0, Arena ar, hipStream_t st, bool precise = false, const sf_visual_fold64* fold64 = nullptr);
int visual_bwd_i(const sf_visual_w* w, const sf_visual_g* g, const PanoSrc& X, int B, int H, int D,
                 const float* h, const float* alpha, const float* t_v, const float* dout, int lddo,
                 const Dropout& drop, int col0, float* dh, Arena ar, hipStream_t st,
                 float* dq_out = nullptr, float* dt_out = nullptr,
                 const SmallPlan* beside = nullptr,     // an independent small product to launch with
                 int dout_slabs = 0, long dout_slab_stride = 0);   // dout = the sum of K-split slabs (added up in the kernel)
// h lives in cat2[:, H:2H] already (copy_from != null copies it there first).
int softdot_fwd_i(const sf_softdot_w* w, int B, int L, int H, const float* copy_from, int ldh,
                  const float* ctx, const uint8_t* mask, float* h_tilde, float* alpha, float* cat2,
                  float* t_text, Arena ar, hipStream_t st, const int32_t* ctx_row = nullptr);
int softdot_bwd_i(const sf_softdot_w* w, const sf_softdot_g* g, int B, int L, int H,
                  const float* ctx, const float* alpha, const float* cat2, const float* t_text,
                  const float* h_tilde, const float* dh_tilde, float* dh, int lddh, float* dctx,
                  Arena ar, hipStream_t st, float* dpre_out = nullptr, float* dt_out = nullptr,
                  bool dpre_ready = false,     // dh_tilde already IS dpre (written to dpre_out)
                  float* dcat2_out = nullptr, float* ds_out = nullptr,     // both: dctx is deferred
                  const int32_t* ctx_row = nullptr);                      // (deferred only) row b reads ctx row ctx_row[b]
int scoring_fwd_i(const sf_scoring_w* w, const CandSrc& U, int B, int H, int D, const float* h,
                  float* logit, float* t_a, float* wt, float* r, Arena ar, hipStream_t st,
                  const sf_follower_glue* glue = nullptr, bool t_a_done = false);     // t_a / wt already formed by the caller (paired launch)
int scoring_bwd_i(const sf_scoring_w* w, const sf_scoring_g* g, const CandSrc& U, int B, int H,
                  int D, const float* h, const float* t_a, const float* wt, const float* dlogit,
                  float* dh, Arena ar, hipStream_t st, const sf_decoder_gtape* gt = nullptr,
                  const float* tanh_of = nullptr, bool* tanh_done = nullptr,
                  const CeSrc* ce = nullptr);

}  // namespace sf
