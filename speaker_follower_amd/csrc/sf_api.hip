// extern "C" entry points of libsf_hip.so (see include/sf_hip.h) and the host-side sequencing of
// kernels for the composite operators.  Nothing here allocates or synchronises.
#include "sf_kernels.h"
#include "sf_gemm_small.h"
#include "sf_glue.h"

using namespace sf;

#include <atomic>
#include <climits>
#include <map>
#include <mutex>
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
}  // namespace sf

namespace {

constexpr size_t WORKSPACE_BYTES = 64u << 20;
// the weight-gradient entry points take a LARGER scratch buffer when the caller has one (the grouped weight gradients keep
// ~135 MB of transposed operands + slabs); kept apart from the workspace of the decode steps: measured in round 5, a
// 256 MB workspace costs the headline rollout 2 % (1.02 vs 1.04 M agent-steps/s, same kernels, same box)
constexpr size_t WGRAD_WORKSPACE_BYTES = 256u << 20;

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

// ---- fp16 storage of the feature table (include/sf_hip.h: sf_feature_table_f16) ----------------------------------------
// The C structs carry no storage tag (ABI 9 pins their layout): a table is known to hold binary16 by its ADDRESS.
constexpr int F16_TABLES = 16;
const void* g_f16_tables[F16_TABLES];
int g_f16_ntables = 0;
std::mutex g_f16_mutex;
int table_is_f16(const void* table) {
    if (!table) return 0;
    std::lock_guard<std::mutex> lock(g_f16_mutex);
    for (int i = 0; i < g_f16_ntables; ++i)
        if (g_f16_tables[i] == table) return 1;
    return 0;
}

// ---- projected feature tables (include/sf_hip.h: sf_projected_register) -------------------------------------------------
// Like the storage tag above, the tables reach the library by the ADDRESS of the feature table they were built from: no
// struct of ABI 9 changes layout.  One entry per table; an entry also names the decoder it belongs to (two of its weights)
// and the location table, and a step whose decoder or location table is another one does not see it.
constexpr int PROJ_TABLES = 16;
struct ProjEntry { const void* table; sf_projected p; };
ProjEntry g_proj[PROJ_TABLES];
int g_proj_n = 0;
std::mutex g_proj_mutex;
std::atomic<int> g_proj_use{1};             // sf_projected_use
std::atomic<long long> g_proj_steps{0};     // sf_projected_steps: decode steps issued on the projected chain
static int g_proj_partials_late = 0;        // sf_debug_projected_partials_late (0: the attention partials in launch (1))
bool projected_lookup(const void* table, sf_projected* out) {
    if (!table || !g_proj_use.load(std::memory_order_relaxed)) return false;
    std::lock_guard<std::mutex> lock(g_proj_mutex);
    for (int i = 0; i < g_proj_n; ++i)
        if (g_proj[i].table == table) {
            *out = g_proj[i].p;
            return true;
        }
    return false;
}
inline int projected_ld(int H) { return (H + 1 + 3) & ~3; }

// ---- gate-space rows (include/sf_hip.h: sf_gate_rows_register) --------------------------------------------------------------
// The same registration by the feature table's ADDRESS; an entry names the decoder by its W_ih.
constexpr int GATE_TABLES = 16;
struct GateEntry { const void* table; sf_gate_rows g; };
GateEntry g_gate[GATE_TABLES];
int g_gate_n = 0;
std::mutex g_gate_mutex;
std::atomic<int> g_gate_use{1};             // sf_gate_rows_use
std::atomic<long long> g_gate_steps{0};     // sf_gate_rows_steps: decode steps whose gate product ran on a gate-space row
bool gate_rows_lookup(const void* table, sf_gate_rows* out) {
    if (!table || !g_gate_use.load(std::memory_order_relaxed)) return false;
    std::lock_guard<std::mutex> lock(g_gate_mutex);
    for (int i = 0; i < g_gate_n; ++i)
        if (g_gate[i].table == table) {
            *out = g_gate[i].g;
            return true;
        }
    return false;
}

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

#define TRY(expr)                     \
    do {                              \
        int _st = (expr);             \
        if (_st != SF_OK) return _st; \
    } while (0)
#define NEED(ptr) \
    if (!(ptr)) return SF_ERR_WORKSPACE

// b_ih and b_hh of an LSTM have the same gradient (the column sums of dgates): one pass, two outputs
int colsum_pair(const float* Y, int ldy, int M, int N, float* a, float* b, Arena ar, hipStream_t st) {
    float* first = a ? a : b;
    if (!first) return SF_OK;
    return colsum(Y, ldy, M, N, first, 1, st, (a && b) ? b : nullptr, ar.rest(), ar.rest_n());
}

int linear_plain(const float* x, int ldx, const float* w, int ldw, const float* b, int M, int N,
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
int data_grad(const float* dy, int lddy, const float* w, const float* w_t, int M, int N, int K,
              float* dx, int lddx, int accumulate, Arena ar, hipStream_t st) {
    if (w_t && N % 4 == 0) {
        Seg sg{dy, lddy, w_t, N, N};
        LinearOut o{};
        o.y = dx; o.ldy = lddx; o.epi = EPI_NONE; o.accumulate = accumulate;
        return linear_nt(&sg, 1, M, K, o, ar.rest(), ar.rest_n(), st);
    }
    return gemm_nn_ws(dy, lddy, w, K, M, K, N, dx, lddx, accumulate, ar.rest(), ar.rest_n(), st);
}

// ---- bf16 weight storage of the gate product (include/sf_hip.h: sf_gate_product_bf16_weights) ---------------------------
std::atomic<int> g_bf16w_on{0};
struct Bf16Pair { const float* w_ih; const float* w_hh; const void* p_ih; const void* p_hh; };
constexpr int BF16_PAIRS = 16;
Bf16Pair g_bf16_pairs[BF16_PAIRS];
int g_bf16_npairs = 0;
std::mutex g_bf16_mutex;

// the packed images of (w_ih, w_hh) when the switch is on and the pair is registered; false: today's kernels
bool bf16_packed(const float* w_ih, const float* w_hh, const void* (&packed)[2]) {
    if (!g_bf16w_on.load(std::memory_order_relaxed) || sf::g_nt_force_f32) return false;
    std::lock_guard<std::mutex> lock(g_bf16_mutex);
    for (int i = 0; i < g_bf16_npairs; ++i)
        if (g_bf16_pairs[i].w_ih == w_ih && g_bf16_pairs[i].w_hh == w_hh) {
            packed[0] = g_bf16_pairs[i].p_ih;
            packed[1] = g_bf16_pairs[i].p_hh;
            return true;
        }
    return false;
}

// ---- a2 LSTMCell --------------------------------------------------------------------------------
int lstm_fwd_i(const sf_lstm_w* w, int B, int I, int H, const float* x, int ldx, const float* h0,
               const float* c0, float* h1, float* c1, float* gates, float* h1_drop, int ld_h1_drop,
               const Dropout& drop, Arena ar, hipStream_t st,
               const float* xg = nullptr, int x_col0 = 0) {     // xg [B, 4H]: x[:, :x_col0] W_ih[:, :x_col0]^T, formed elsewhere
    LstmPwFwd p{};                                              // (the product then starts at column x_col0 of x and W_ih)
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

static int g_slab_consumers = 1;     // sf_debug_slab_consumers: consumers add up K-split slabs themselves (0: a reduce launch in between)

int lstm_bwd_i(const sf_lstm_w* w, const sf_lstm_g* g, int B, int I, int H, const float* x, int ldx,
               const float* h0, const float* c0, const float* c1, const float* gates,
               const float* dh1, const float* dh1_b, const float* dc1, float* dx, int lddx,
               float* dh0, float* dc0, Arena ar, hipStream_t st, float* dgates_out = nullptr,
               int dx_col0 = 0,            // dx is only formed for input columns >= dx_col0
               const Dropout* dh1b_drop = nullptr,     // mask still to be applied to dh1_b
               SmallPlan* dh0_plan = nullptr, bool* dh0_deferred = nullptr,
               const float** dx_slabs = nullptr, int* dx_ks = nullptr) {   // (with dx_col0 > 0) leave d(x[:, dx_col0:]) as the
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
                 int col0, Arena ar, hipStream_t st, bool precise = false, const sf_visual_fold64* fold64 = nullptr) {
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
                 float* dq_out = nullptr, float* dt_out = nullptr,
                 const SmallPlan* beside = nullptr,     // an independent small product to launch with
                 int dout_slabs = 0, long dout_slab_stride = 0) {   // dout = the sum of K-split slabs (added up in the kernel)
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
// h lives in cat2[:, H:2H] already (copy_from != null copies it there first).
int softdot_fwd_i(const sf_softdot_w* w, int B, int L, int H, const float* copy_from, int ldh,
                  const float* ctx, const uint8_t* mask, float* h_tilde, float* alpha, float* cat2,
                  float* t_text, Arena ar, hipStream_t st, const int32_t* ctx_row = nullptr) {
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
                  Arena ar, hipStream_t st, float* dpre_out = nullptr, float* dt_out = nullptr,
                  bool dpre_ready = false,     // dh_tilde already IS dpre (written to dpre_out)
                  float* dcat2_out = nullptr, float* ds_out = nullptr,     // both: dctx is deferred
                  const int32_t* ctx_row = nullptr) {                      // (deferred only) row b reads ctx row ctx_row[b]
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
                  const sf_follower_glue* glue = nullptr, bool t_a_done = false) {     // t_a / wt already formed by the caller (paired launch)
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
                  float* dh, Arena ar, hipStream_t st, const sf_decoder_gtape* gt = nullptr,
                  const float* tanh_of = nullptr, bool* tanh_done = nullptr,
                  const CeSrc* ce = nullptr) {
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

}  // namespace

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
size_t sf_pack_bf16_bytes(int rows, int K) { return sf::pack_bf16_bytes(rows, K); }
int sf_pack_bf16(const float* w, int ld, int rows, int K, void* out, sf_stream stream) {
    SF_ENTER();
    return sf::pack_bf16(w, ld, rows, K, out, S(stream));
}
int sf_lstm_weights_bf16(const float* w_ih, const float* w_hh, const void* packed_ih, const void* packed_hh) {
    SF_CHECK_ARG(w_ih && (packed_ih || !packed_hh) && (!packed_ih || !w_hh == !packed_hh));
    std::lock_guard<std::mutex> lock(g_bf16_mutex);
    int at = -1;
    for (int i = 0; i < g_bf16_npairs; ++i)
        if (g_bf16_pairs[i].w_ih == w_ih && g_bf16_pairs[i].w_hh == w_hh) at = i;
    if (!packed_ih) {                                           // forget the pair (unknown: nothing to do)
        if (at >= 0) g_bf16_pairs[at] = g_bf16_pairs[--g_bf16_npairs];
        return SF_OK;
    }
    if (at < 0) {
        if (g_bf16_npairs == BF16_PAIRS) return SF_ERR_UNSUPPORTED;
        at = g_bf16_npairs++;
    }
    g_bf16_pairs[at] = Bf16Pair{w_ih, w_hh, packed_ih, packed_hh};
    return SF_OK;
}
int sf_feature_table_f16(const void* table, int on) {
    SF_CHECK_ARG(table);
    std::lock_guard<std::mutex> lock(g_f16_mutex);
    int at = -1;
    for (int i = 0; i < g_f16_ntables; ++i)
        if (g_f16_tables[i] == table) at = i;
    if (!on) {                                                  // forget the address (unknown: nothing to do)
        if (at >= 0) g_f16_tables[at] = g_f16_tables[--g_f16_ntables];
        return SF_OK;
    }
    if (at >= 0) return SF_OK;
    if (g_f16_ntables == F16_TABLES) return SF_ERR_UNSUPPORTED;
    g_f16_tables[g_f16_ntables++] = table;
    return SF_OK;
}
int sf_feature_table_is_f16(const void* table) { return table_is_f16(table); }
int sf_projected_ld(int H) { return H > 0 ? projected_ld(H) : 0; }
int sf_projected_register(const void* table, const sf_projected* p) {
    SF_CHECK_ARG(table);
    if (p)
        SF_CHECK_ARG(p->pv && p->pa && p->lv && p->la && p->loc_table && p->key_v && p->key_a && p->H > 0 && p->H % 4 == 0 &&
                     p->ld == projected_ld(p->H) && p->V > 0 && p->IMG > 0 && p->LOC > 0);
    std::lock_guard<std::mutex> lock(g_proj_mutex);
    int at = -1;
    for (int i = 0; i < g_proj_n; ++i)
        if (g_proj[i].table == table) at = i;
    if (!p) {                                                   // forget the address (unknown: nothing to do)
        if (at >= 0) g_proj[at] = g_proj[--g_proj_n];
        return SF_OK;
    }
    if (at < 0) {
        if (g_proj_n == PROJ_TABLES) return SF_ERR_UNSUPPORTED;
        at = g_proj_n++;
    }
    g_proj[at] = ProjEntry{table, *p};
    return SF_OK;
}
int sf_projected_registered(const void* table, sf_projected* out) {
    std::lock_guard<std::mutex> lock(g_proj_mutex);
    for (int i = 0; i < g_proj_n; ++i)
        if (table && g_proj[i].table == table) {
            if (out) *out = g_proj[i].p;
            return 1;
        }
    return 0;
}
void sf_projected_use(int on) { g_proj_use.store(on ? 1 : 0, std::memory_order_relaxed); }
int sf_projected_is_used(void) { return g_proj_use.load(std::memory_order_relaxed); }
long long sf_projected_steps(void) { return g_proj_steps.load(std::memory_order_relaxed); }
void sf_debug_projected_partials_late(int on) { g_proj_partials_late = on; }
void sf_debug_projected_text_groups(int groups) { sf::g_proj_text_groups = groups == 2 || groups == 4 ? groups : 0; }
int sf_projected_text_groups_plan(int B, int L, int with_partials, int slots, int product_blocks, int* grid) {
    if (B < 1 || L < 1 || slots < 0 || product_blocks < 0) return 0;
    return sf::proj_text_groups_plan(B, L, with_partials != 0, product_blocks, slots, 0, grid);
}
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
// rows of the feature table one product of the build takes (its output, the largest thing in flight, is 34 MB)
constexpr long long PROJ_CHUNK_ROWS = 16384;
static long long g_proj_chunk_rows = PROJ_CHUNK_ROWS;      // sf_debug_projected_chunk_rows
void sf_debug_projected_chunk_rows(int rows) { g_proj_chunk_rows = rows > 0 ? rows : PROJ_CHUNK_ROWS; }
// the shape test of the chain (proj_chain_supported) for a caller that has not built anything yet: 1 when a step of this
// shape on index-form fp32 rows can take the chain (the small-product plan of y is still the step's to check)
int sf_projected_supported(int B, int H, int L, int A, int V, int IMG, int LOC) {
    if (H <= 0 || IMG <= 0 || LOC <= 0 || V <= 0) return 0;
    static const float dummy[4] = {0.f, 0.f, 0.f, 0.f};
    static const int idummy[1] = {0};
    CandSrc us{};
    us.table = dummy; us.a_num = idummy; us.A = A; us.V = V; us.IMG = IMG; us.LOC = LOC;
    PanoSrc xn{};
    xn.table = dummy; xn.V = V; xn.IMG = IMG; xn.LOC = LOC;
    const ProjTables pt{dummy, dummy, dummy, dummy, projected_ld(H), H};
    return proj_chain_supported(us, &xn, B, H, L, pt) ? 1 : 0;
}
int sf_projected_build(const sf_decoder_fold* fold, const float* table, long long n_rows, const float* loc_table, int V, int IMG,
                       int LOC, int H, float* pv, float* pa, float* lv, float* la, void* ws, size_t ws_bytes,
                       sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(fold && fold->m_v && fold->c_v && fold->m_a && fold->c_a && table && loc_table && pv && pa && lv && la &&
                 n_rows > 0 && V > 0 && IMG > 0 && IMG % 4 == 0 && LOC > 0 && LOC % 16 == 0 && H > 0 && H % 4 == 0);
    if (table_is_f16(table)) return SF_ERR_UNSUPPORTED;
    const int F = IMG + LOC, Fa = F + 4, ld = projected_ld(H), Ks = LOC + 4, g = LOC / 4;
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    sf::proj_text_slots_warm();       // (launch (1)'s group rule reads the device once, here: never inside a capture)
    // the folds transposed to the [N, K] layout of the products below, the constant as row H, zero rows up to ld:
    //   wt_v [ld, F]     = [M_v^T ; c_v ; 0]
    //   wt_a [ld, F + 4] = [M_a^T ; c_a ; 0]   (column F of M_a^T is m, c_a[F] is c0: sf_decoder_fold_build)
    float* wt_v = ar.take((size_t)ld * F);
    float* wt_a = ar.take((size_t)ld * Fa);
    float* sel = ar.take((size_t)5 * Ks);      // rows 0..3: ones over block g of the location part; row 4: one at column F
    NEED(wt_v && wt_a && sel);
    TRY(fill(wt_v + (size_t)H * F, (size_t)(ld - H) * F, 0.f, st));
    TRY(fill(wt_a + (size_t)H * Fa, (size_t)(ld - H) * Fa, 0.f, st));
    TRY(transpose(fold->m_v, F, H, wt_v, st));
    TRY(transpose(fold->m_a, Fa, H, wt_a, st));
    TRY(add2(fold->c_v, F, nullptr, 0, 1, F, wt_v + (size_t)H * F, F, st));
    TRY(add2(fold->c_a, Fa, nullptr, 0, 1, Fa, wt_a + (size_t)H * Fa, Fa, st));
    TRY(fill(sel, (size_t)5 * Ks, 0.f, st));
    for (int q = 0; q < 4; ++q) TRY(fill(sel + (size_t)q * Ks + (size_t)q * g, (size_t)g, 1.f, st));
    TRY(fill(sel + (size_t)4 * Ks + LOC, 1, 1.f, st));
    // the two large tables, PROJ_CHUNK_ROWS rows of the feature table per product (64-bit row offsets; the products write
    // straight into the tables: no temporary beyond the transposed folds above)
    for (long long r0 = 0; r0 < n_rows; r0 += g_proj_chunk_rows) {
        const int m = (int)std::min<long long>(g_proj_chunk_rows, n_rows - r0);
        const float* x = table + (size_t)r0 * IMG;
        TRY(linear_plain(x, IMG, wt_v, F, nullptr, m, ld, IMG, EPI_NONE, pv + (size_t)r0 * ld, ld, ar, st));
        TRY(linear_plain(x, IMG, wt_a, Fa, nullptr, m, ld, IMG, EPI_NONE, pa + (size_t)r0 * ld, ld, ar, st));
    }
    TRY(linear_plain(loc_table, LOC, wt_v + IMG, F, nullptr, V * V, ld, LOC, EPI_NONE, lv, ld, ar, st));
    return linear_plain(sel, Ks, wt_a + IMG, Fa, nullptr, 5, ld, Ks, EPI_NONE, la, ld, ar, st);
}
int sf_gate_rows_build(const float* w_ih, const float* table, long long n_rows, int IMG, int LOC, int H, float* gu, float* gl,
                       void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w_ih && table && gu && gl && n_rows > 0 && IMG > 0 && IMG % 4 == 0 && LOC > 0 && LOC % 16 == 0 && H > 0 &&
                 H % 4 == 0);
    if (table_is_f16(table)) return SF_ERR_UNSUPPORTED;
    const int F = IMG + LOC, G = 4 * H, g = LOC / 4;
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    float* sel = ar.take((size_t)4 * LOC);      // row k: ones over block k of the location part
    NEED(sel);
    TRY(fill(sel, (size_t)4 * LOC, 0.f, st));
    for (int q = 0; q < 4; ++q) TRY(fill(sel + (size_t)q * LOC + (size_t)q * g, (size_t)g, 1.f, st));
    // gu, PROJ_CHUNK_ROWS rows of the feature table per product against the leading IMG columns of W_ih [4H, 2F] (64-bit
    // row offsets; the products write straight into the table)
    for (long long r0 = 0; r0 < n_rows; r0 += g_proj_chunk_rows) {
        const int m = (int)std::min<long long>(g_proj_chunk_rows, n_rows - r0);
        TRY(linear_plain(table + (size_t)r0 * IMG, IMG, w_ih, 2 * F, nullptr, m, G, IMG, EPI_NONE, gu + (size_t)r0 * G, G, ar, st));
    }
    return linear_plain(sel, LOC, w_ih + IMG, 2 * F, nullptr, 4, G, LOC, EPI_NONE, gl, G, ar, st);
}
int sf_gate_rows_register(const void* table, const sf_gate_rows* g) {
    SF_CHECK_ARG(table);
    if (g) SF_CHECK_ARG(g->gu && g->gl && g->key_w && g->H > 0 && g->H % 4 == 0 && g->V > 0 && g->IMG > 0 && g->LOC > 0);
    std::lock_guard<std::mutex> lock(g_gate_mutex);
    int at = -1;
    for (int i = 0; i < g_gate_n; ++i)
        if (g_gate[i].table == table) at = i;
    if (!g) {                                                   // forget the address (unknown: nothing to do)
        if (at >= 0) g_gate[at] = g_gate[--g_gate_n];
        return SF_OK;
    }
    if (at < 0) {
        if (g_gate_n == GATE_TABLES) return SF_ERR_UNSUPPORTED;
        at = g_gate_n++;
    }
    g_gate[at] = GateEntry{table, *g};
    return SF_OK;
}
int sf_gate_rows_registered(const void* table, sf_gate_rows* out) {
    std::lock_guard<std::mutex> lock(g_gate_mutex);
    for (int i = 0; i < g_gate_n; ++i)
        if (table && g_gate[i].table == table) {
            if (out) *out = g_gate[i].g;
            return 1;
        }
    return 0;
}
void sf_gate_rows_use(int on) { g_gate_use.store(on ? 1 : 0, std::memory_order_relaxed); }
int sf_gate_rows_is_used(void) { return g_gate_use.load(std::memory_order_relaxed); }
long long sf_gate_rows_steps(void) { return g_gate_steps.load(std::memory_order_relaxed); }
void sf_gate_product_bf16_weights(int on) { g_bf16w_on.store(on ? 1 : 0, std::memory_order_relaxed); }
int sf_gate_product_bf16_weights_is_on(void) { return g_bf16w_on.load(std::memory_order_relaxed); }
int sf_gate_product_bf16_supported(int M, int K1, int K2, int N) {
    if (K2 < 0) return 0;
    const int K[2] = {K1, K2};
    return sf::bf16w_supported(M, N, K, K2 ? 2 : 1) ? 1 : 0;
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

// ---- a6, software-pipelined across steps ---------------------------------------------------------------
// head(t)   = visual half of step t: t_v, q, visual attention -> tape->xin[:, F:2F], alpha_v
// tail(t)   = LSTM cell, text attention, scoring (+ glue) of step t, and -- when X_next is given --
//             head(t+1) on h1 of step t, run SIDE BY SIDE with the text / scoring half in paired
//             launches (sf_attention.hip): the two halves are independent given h1.
static int decoder_head_a(const sf_decoder_w* w, const sf_pano* X, int B, int H, int D,
                          const float* h0, const sf_decoder_tape* tp, const sf_dropout* drop,
                          uint32_t step_id, Arena ar, sf_stream stream) {
    SF_CHECK_ARG(w && X && h0 && tp && B > 0);
    const PanoSrc xs = pano(X);
    const int F = xs.IMG + xs.LOC;
    return visual_fwd_i(&w->visual, xs, B, H, D, h0, tp->xin + F, 2 * F, tp->alpha_v, tp->t_v, tp->q,
                        make_dropout(drop, 2 * step_id, 2), F, ar, S(stream));
}

int sf_attn_decoder_head_fwd(const sf_decoder_w* w, const sf_pano* X, int B, int H, int D,
                             const float* h0, const sf_decoder_tape* tp, const sf_dropout* drop,
                             uint32_t step_id, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    return decoder_head_a(w, X, B, H, D, h0, tp, drop, step_id, arena(ws, ws_bytes), stream);
}

static int plan_linear(const float* x, int ldx, const float* wgt, int ldw, const float* b, int M,
                       int N, int K, Epi epi, float* y, int ldy, SmallPlan* p) {
    Seg sg{x, ldx, wgt, ldw, K};
    LinearOut o{};
    o.y = y; o.ldy = ldy; o.bias = b; o.epi = epi;
    return linear_small_plan(&sg, 1, M, N, o, p) ? SF_OK : SF_ERR_UNSUPPORTED;
}

// the episode's folded context tensors (sf_follower_episode.ctx_q / ctx_o; sf_attention.hip: text_fold_body)
struct TextFold {
    const float* ctx_q;
    const float* ctx_o;
};

// ---- tail(t): what every launch chain of the step reads (decoder_tail_i builds it behind the cell, tail_dispatch picks
// ONE chain).  A chain is a function of two parts: a PLAN that launches nothing (plan_linear / linear_small_plan, scratch
// takes, shape limits) and the ISSUE of its launches.  So SF_ERR_UNSUPPORTED from a chain means "nothing was launched,
// try the next chain" -- never a half-issued step -- and any other status ends the step.
struct TailStep {
    const sf_decoder_w* w;
    CandSrc us;
    int B, H, D, L, F;
    const sf_decoder_tape *tp, *tn;     // the tape of this step; of the next one (null: nothing of it is prepared here)
    const sf_follower_glue* glue;
    Dropout d_h, dn_in;                 // of h1 (into cat2[:, H:]); of the next step's LSTM input
    PanoSrc xn;                         // the panorama of the next step, where `has_xn`
    bool has_xn;
    bool paired, query_only, last_step;
    const float* ctx;
    const uint8_t* ctx_mask;
    const int32_t* ctx_row;
    Arena ar;
    hipStream_t st;
    struct GateStep* gate;              // gate-space rows of the episode (null: none), see GateStep
};

// Gate-space rows through one step (sf_follower_episode_fwd): `xg_in` is the row the step before left for this step's cell
// (null: the full gate product), `rows.xg_next` where launch (2) of the projected chain leaves the next one; `wrote` says
// whether it did -- any other chain writes the raw u_next alone, and the next step runs the full product.
struct GateStep {
    const float* xg_in;
    GateRows rows;
    bool wrote;
};

// a launch BEHIND a chain's first one: the step is half issued, "unsupported" can no longer mean "try the next chain"
static inline int issued(int rc) { return rc == SF_ERR_UNSUPPORTED ? SF_ERR_LAUNCH : rc; }

// the second body of a paired launch left empty (no next step to prepare)
static SmallPlan empty_plan(SmallPlan p) {
    p.gx = p.gy = 0;
    return p;
}

// the visual attention of step t+1 on its query tn->q -- beside the small product `b` (phases: pair_vis_small) ...
static int vis_next_beside(const TailStep& s, float* part, unsigned* counter, const SmallPlan& b, int phase = 0) {
    return pair_vis_small(s.xn, s.B, s.tn->q, s.F, s.tn->alpha_v, s.tn->xin + s.F, 2 * s.F, s.dn_in, s.F, part, counter, b,
                          s.st, phase);
}
// ... or as a launch of its own
static int vis_next_alone(const TailStep& s, float* part, const Arena& ar) {
    return visual_attn(0, s.xn, s.B, s.tn->q, s.F, s.tn->alpha_v, s.tn->xin + s.F, 2 * s.F, s.dn_in, s.F, s.st, part,
                       part ? ar.tickets() : nullptr);
}

static int score_tail(const TailStep& s, const Arena& ar, bool t_a_done = false) {
    const sf_decoder_tape* tp = s.tp;
    return scoring_fwd_i(&s.w->action, s.us, s.B, s.H, s.D, tp->h_tilde, tp->logit, tp->t_a, tp->wt, tp->r, ar, s.st, s.glue,
                         t_a_done);
}

// scratch of the two folded chains
struct FoldScratch {
    float *tpart, *ybuf, *zbuf, *part;
    unsigned* tcount;
    int ldp;
    bool ok;         // everything was there, and B within the split attention's limit
};
// `af` is the chain's own COPY of the step's arena: a chain that declines hands the whole workspace to the next one
// (B = 300 fits only because of this).
static FoldScratch fold_scratch(const TailStep& s, Arena& af) {
    FoldScratch f{};
    f.tpart = af.take(text_fold_part_floats(s.B, s.H));
    // (leading dimension H + 16: rows of a power-of-two stride share a few cache sets, CHANGELOG round 5 "2c")
    f.ldp = s.H + 16;
    f.ybuf = af.take((size_t)s.B * f.ldp);
    f.zbuf = af.take((size_t)s.B * f.ldp);
    f.tcount = af.tickets() ? af.tickets() + TEXT_TICKET : nullptr;
    f.part = (s.paired && s.B <= 1024) ? af.take(visual_attn_split_floats(s.B, s.F)) : nullptr;
    f.ok = f.tpart && f.ybuf && f.zbuf && (f.part || !s.paired) && f.tcount && s.B <= VIS_SPLIT_MAX_B;
    return f;
}

// the last launch of the four-launch folded chain: logit = u . r + the biases through wt -- with the glue and the merge of
// the next step's attention partials `merge_part` in the same launch, with the glue alone, or bare
static int fold_score(const TailStep& s, float* merge_part) {
    const sf_scoring_w& a = s.w->action;
    const sf_decoder_tape* tp = s.tp;
    if (merge_part)
        return pair_score_merge(s.us, s.B, s.D, tp->r, tp->wt, a.b_a, a.b_out, make_glue(s.us, s.B, tp->logit, s.glue), s.xn,
                                s.tn->alpha_v, s.tn->xin + s.F, 2 * s.F, s.dn_in, s.F, merge_part, s.st);
    if (s.glue)
        return score_glue_fwd(s.us, s.B, s.D, tp->r, tp->wt, a.b_a, a.b_out, make_glue(s.us, s.B, tp->logit, s.glue), s.st);
    return score_fwd(s.us, s.B, s.D, tp->r, tp->wt, a.b_a, a.b_out, tp->logit, s.st);
}

// Projected chain (inference; tables of sf_projected_build registered for the step's feature table and decoder): TWO
// dependent launches behind the cell --
//   (1) folded text attention  ||  y = W_out[:, H:] h1  ||  attention partials of step t+1, scores from projected rows and h1
//   (2) scoring + glue on projected candidate rows, h~ = tanh(z + y) formed in the body  ||  merge of the partials
// q, t_v', t_a, wt and r are never formed (and their tape slots not written: nothing runs backward through this step).
// PLACEMENT of the partials (sf_debug_projected_partials_late, default 0): in (1), beside the text stage.  They need only
// h1, not the text attention or the chosen action, so there they leave the chain cell -> text -> score -> next gate
// product; (2) keeps their merge.  Their body (sf_attention.hip: proj_partials_body) fits 128 registers per lane, so the
// grid of (1) runs two 512-thread workgroups per CU: measured at B = 100, (1) 18.7 us + (2) 7.4 us against 10.3 us +
// 18.0 us with partials, ticket and merge in (2) (pair_proj_score_kernel<0>), 1.429 against 1.474 ms per rollout
// (profiles/partials_early_ab.txt).  With visual_split_body's ~190 registers in (1) -- one workgroup per CU for every block
// of that grid -- it was 23.6 us + 7.3 us and the late placement won.  A panorama whose row layout the body does not take
// (proj_partials_supported) keeps the late placement.
// the registered tables of (candidate table, decoder) where the chain's shapes hold for them (xn: the panorama whose
// attention rides along, or null)
static bool projected_for(const sf_decoder_w* w, const CandSrc& us, const PanoSrc* xn, int B, int H, int L, ProjTables* pt) {
    sf_projected reg;
    if (us.dense || us.half || !projected_lookup(us.table, &reg)) return false;
    if (reg.key_v != w->visual.w_h || reg.key_a != w->action.w_h || reg.V != us.V || reg.IMG != us.IMG || reg.LOC != us.LOC ||
        (xn && xn->loc_table != reg.loc_table))
        return false;
    *pt = ProjTables{reg.pv, reg.pa, reg.lv, reg.la, reg.ld, reg.H};
    return proj_chain_supported(us, xn, B, H, L, *pt);
}

static int tail_proj(const TailStep& s, const TextFold& tf) {
    const sf_decoder_tape *tp = s.tp, *tn = s.tn;
    const int B = s.B, H = s.H, F = s.F;
    // ---- plan
    ProjTables pt;
    if (!s.glue || s.query_only || !(s.paired || s.last_step) ||
        !projected_for(s.w, s.us, s.paired ? &s.xn : nullptr, B, H, s.L, &pt))
        return SF_ERR_UNSUPPORTED;
    Arena af = s.ar;
    const FoldScratch f = fold_scratch(s, af);
    SmallPlan py;
    const bool ok = f.ok &&
        plan_linear(tp->cat2 + H, 2 * H, s.w->text.w_out + H, 2 * H, nullptr, B, H, H, EPI_NONE, f.ybuf, f.ldp, &py) == SF_OK &&
        pair_proj_textfold_accepts(py.inst()) && (!s.paired || af.tickets());
    if (!ok) return SF_ERR_UNSUPPORTED;
    // ---- issue (the first launch checks its shapes before it launches: it may still decline)
    const bool late = s.paired && (g_proj_partials_late || !proj_partials_supported(s.xn.IMG, s.xn.LOC));
    TRY(pair_proj_textfold(tf.ctx_q, tf.ctx_o, s.ctx_mask, B, s.L, H, tp->cat2 + H, 2 * H, f.tpart, f.tcount, f.zbuf, f.ldp,
                           tp->alpha, py, s.us, s.paired && !late ? &s.xn : nullptr, pt, tp->h1, H, f.part, s.st));
    g_proj_steps.fetch_add(1, std::memory_order_relaxed);
    const bool gate = s.gate && s.gate->rows.xg_next && s.paired;       // (a next step exists and reads the row)
    TRY(issued(pair_proj_score(s.us, B, H, s.L, pt, f.zbuf, f.ldp, f.ybuf, f.ldp, make_glue(s.us, B, tp->logit, s.glue),
                               s.paired ? &s.xn : nullptr, late ? 0 : 2, tp->h1, H, s.paired ? tn->alpha_v : nullptr,
                               s.paired ? tn->xin + F : nullptr, 2 * F, s.dn_in, F, f.part, af.tickets(), s.st,
                               gate ? &s.gate->rows : nullptr)));
    if (gate) s.gate->wrote = true;
    return SF_OK;
}

// Folded text stage (inference; sf_attention.hip: text_fold_body): FOUR dependent launches behind the cell
// instead of six:
//   (1) folded text attention (4 groups per sample, merged by the last arriver)  ||  y = W_out[:, H:] h1  ||  t_v' = W_h h1 + b_h
//   (2) t_a = W_h tanh(z + y) + b_h, wt = t_a * w_out (A-prologue)   ||  q' = W_v^T t_v'
//   (3) r = W_a^T wt            ||  visual attention of step t+1 (partials, ticket, merge by the last arriver)
//   (4) scoring + glue
// (query_only -- a device-resident environment: the panorama of step t+1 is not known yet -- stage (3) is the
// r product alone and the attention follows the environment step, sf_attn_decoder_attend_fwd)
static int tail_fold4(const TailStep& s, const TextFold& tf) {
    const sf_visual_w* vw = &s.w->visual;
    const sf_scoring_w* aw = &s.w->action;
    const sf_decoder_tape *tp = s.tp, *tn = s.tn;
    const int B = s.B, H = s.H, D = s.D, F = s.F;
    // ---- plan
    Arena af = s.ar;
    const FoldScratch f = fold_scratch(s, af);
    SmallPlan py, pv, pta, pq, pr;
    bool ok = f.ok &&
        plan_linear(tp->cat2 + H, 2 * H, s.w->text.w_out + H, 2 * H, nullptr, B, H, H, EPI_NONE, f.ybuf, f.ldp, &py) == SF_OK &&
        plan_linear(tp->wt, D, aw->w_a_t, D, nullptr, B, F, D, EPI_NONE, tp->r, F, &pr) == SF_OK;
    if (ok && !s.last_step) {
        ok = plan_linear(tp->h1, H, vw->w_h, H, vw->b_h, B, D, H, EPI_NONE, tn->t_v, D, &pv) == SF_OK &&
             plan_linear(tn->t_v, D, vw->w_v_t, D, nullptr, B, F, D, EPI_NONE, tn->q, F, &pq) == SF_OK;
    } else if (ok) {                                       // no next step: the second bodies of (1) and (2) are empty
        pv = empty_plan(py);
        pq = empty_plan(pr);
    }
    if (ok) {
        Seg sg{f.ybuf, f.ldp, aw->w_h, H, H};
        LinearOut o{};
        o.y = tp->wt; o.ldy = D; o.bias = aw->b_h; o.mul = aw->w_out; o.y_pre = tp->t_a;
        o.ldy_pre = D; o.epi = EPI_MUL;
        // (q' and r are both [B, F] over K = D and share one (mt, cpw); stage (3) accepts the same in phases 0 and 1)
        ok = linear_small_plan(&sg, 1, B, D, o, &pta) && pair_apro_small_accepts(pta.inst(), pq.inst()) &&
             pair_vis_small_accepts(pr.inst(), 1);
        pta.args.apro_part = f.zbuf;                            // (the merged attention sum of launch (1))
        pta.args.apro_stride = f.ldp;
    }
    if (!ok) return SF_ERR_UNSUPPORTED;          // (shapes outside the instantiations: the unfolded stages)
    // ---- issue (the first launch checks its shapes before it launches: it may still decline)
    TRY(pair_textfold_small_small(tf.ctx_q, tf.ctx_o, s.ctx_mask, B, s.L, H, tp->cat2 + H, 2 * H, f.tpart, f.tcount, f.zbuf,
                                  f.ldp, tp->alpha, py, pv, s.st));
    TRY(issued(pair_apro_small(pta, pq, s.st)));
    // with a glue: partials beside r, their merge beside the scoring + glue launch (same depth, no in-launch ticket; its
    // shape limits are score_glue_fwd's and pair_vis_small's).  Without one (the module-API step): partials + merge in
    // ONE launch beside r, phase 0
    const bool merge_late = s.paired && s.glue;
    if (merge_late) TRY(issued(vis_next_beside(s, f.part, nullptr, pr, 1)));
    else if (s.paired) TRY(issued(vis_next_beside(s, f.part, af.tickets(), pr, 0)));
    else TRY(issued(launch_small_plan(pr, s.st)));
    return issued(fold_score(s, merge_late ? f.part : nullptr));
}

// Stages (1) and (2) of the unfolded chains, each as one paired launch or -- where that has no instantiation -- as its
// two plain launches (the paired chain and its query-only variant):
//   (1) t_text = W_in dropout(h1)   ||   t_v' = W_h h1 + b_h
//   (2) text attention              ||   q' = W_v^T t_v'
static int text_and_query(const TailStep& s) {
    const sf_softdot_w* tw = &s.w->text;
    const sf_visual_w* vw = &s.w->visual;
    const sf_decoder_tape *tp = s.tp, *tn = s.tn;
    const int B = s.B, H = s.H, D = s.D, L = s.L, F = s.F;
    SmallPlan pa, pb;
    const bool ok1 =
        plan_linear(tp->cat2 + H, 2 * H, tw->w_in, H, nullptr, B, H, H, EPI_NONE, tp->t_text, H, &pa) == SF_OK &&
        plan_linear(tp->h1, H, vw->w_h, H, vw->b_h, B, D, H, EPI_NONE, tn->t_v, D, &pb) == SF_OK;
    if (!ok1 || pair_small_small(pa, pb, s.st) != SF_OK) {
        TRY(linear_plain(tp->cat2 + H, 2 * H, tw->w_in, H, nullptr, B, H, H, EPI_NONE, tp->t_text, H, s.ar, s.st));
        TRY(linear_plain(tp->h1, H, vw->w_h, H, vw->b_h, B, D, H, EPI_NONE, tn->t_v, D, s.ar, s.st));
    }
    const bool ok2 = plan_linear(tn->t_v, D, vw->w_v_t, D, nullptr, B, F, D, EPI_NONE, tn->q, F, &pa) == SF_OK;
    if (!ok2 || pair_small_text(pa, s.ctx, s.ctx_mask, B, L, H, tp->t_text, H, tp->alpha, tp->cat2,
                                2 * H, s.ctx_row, s.st) != SF_OK) {
        TRY(text_attn_fwd(s.ctx, s.ctx_mask, B, L, H, tp->t_text, H, tp->alpha, tp->cat2, 2 * H, s.st, s.ctx_row));
        TRY(linear_plain(tn->t_v, D, vw->w_v_t, D, nullptr, B, F, D, EPI_NONE, tn->q, F, s.ar, s.st));
    }
    return SF_OK;
}

// The paired unfolded chain: (1), (2) above, then
//   (3) h~ = tanh(W_out [wc ; h1])   ||   visual attention of step t+1, per-group partials
//   (4) t_a = W_h h~ + b_h, wt = t_a * w_out   ||   ... merge of the partials
// (the attention is not needed before the next gate product: its two halves ride with two
// stages of the text / scoring chain instead of stretching one of them)
// (never declines: (3) / (4) fall back to h~ beside the whole attention, then to the two plain launches)
static int tail_paired(const TailStep& s) {
    const sf_softdot_w* tw = &s.w->text;
    const sf_scoring_w* aw = &s.w->action;
    const sf_decoder_tape* tp = s.tp;
    const int B = s.B, H = s.H, D = s.D, F = s.F;
    // ---- plan of (3) and (4) ((1) and (2) keep the whole arena, the later stages what the partials leave)
    Arena ar = s.ar;
    float* part = B <= 1024 ? ar.take(visual_attn_split_floats(B, F)) : nullptr;
    SmallPlan ph, pc;
    const bool ok3 = part && plan_linear(tp->cat2, 2 * H, tw->w_out, 2 * H, nullptr, B, H, 2 * H,
                                         EPI_TANH, tp->h_tilde, H, &ph) == SF_OK;
    bool ok4 = false;
    if (ok3) {
        Seg sg{tp->h_tilde, H, aw->w_h, H, H};
        LinearOut o{};
        o.y = tp->wt; o.ldy = D; o.bias = aw->b_h; o.mul = aw->w_out; o.y_pre = tp->t_a;
        o.ldy_pre = D; o.epi = EPI_MUL;
        ok4 = linear_small_plan(&sg, 1, B, D, o, &pc) && pair_vis_small_accepts(pc.inst(), 2);
    }
    // ---- issue
    TRY(text_and_query(s));
    if (ok4 && vis_next_beside(s, part, nullptr, ph, 1) == SF_OK) {
        TRY(vis_next_beside(s, part, nullptr, pc, 2));
        return score_tail(s, ar, true);
    }
    if (!ok3 || vis_next_beside(s, part, ar.tickets(), ph) != SF_OK) {
        TRY(linear_plain(tp->cat2, 2 * H, tw->w_out, 2 * H, nullptr, B, H, 2 * H, EPI_TANH, tp->h_tilde, H, ar, s.st));
        TRY(vis_next_alone(s, part, ar));
    }
    return score_tail(s, ar);
}

// tape_next WITHOUT X_next: the next panorama is not known yet (it depends on this step's action: a
// device-resident environment).  Only the query of the next step's visual attention (t_v', q': they need
// nothing but h1) rides beside the text stages; the attention itself follows the environment step
// (sf_attn_decoder_attend_fwd).
static int tail_query_only(const TailStep& s) {
    const sf_decoder_tape* tp = s.tp;
    TRY(text_and_query(s));
    TRY(linear_plain(tp->cat2, 2 * s.H, s.w->text.w_out, 2 * s.H, nullptr, s.B, s.H, 2 * s.H, EPI_TANH, tp->h_tilde, s.H,
                     s.ar, s.st));
    return score_tail(s, s.ar);
}

// The plain step: text attention and scoring, and -- with a next panorama but no transposed W_v to pair its query
// with -- the whole visual half of step t+1 behind them.
static int tail_plain(const TailStep& s) {
    const sf_decoder_tape *tp = s.tp, *tn = s.tn;
    TRY(softdot_fwd_i(&s.w->text, s.B, s.L, s.H, nullptr, 0, s.ctx, s.ctx_mask, tp->h_tilde, tp->alpha, tp->cat2,
                      tp->t_text, s.ar, s.st, s.ctx_row));
    if (s.has_xn)
        TRY(visual_fwd_i(&s.w->visual, s.xn, s.B, s.H, s.D, tp->h1, tn->xin + s.F, 2 * s.F, tn->alpha_v, tn->t_v, tn->q,
                         s.dn_in, s.F, s.ar, s.st));
    return score_tail(s, s.ar);
}

// The order of preference.  The folded chains (inference: no dropout of h1, no row indirection of the context, the
// episode's TextFold) may decline -- before their first launch, see TailStep -- and hand the step to the next one.
static int tail_dispatch(const TailStep& s, const TextFold* tf) {
    const bool foldable = (s.paired || s.query_only || s.last_step) && tf && !s.ctx_row && !s.d_h.on() && s.w->text.w_out;
    int rc = SF_ERR_UNSUPPORTED;
    if (foldable) rc = tail_proj(s, *tf);
    if (rc == SF_ERR_UNSUPPORTED && foldable && s.w->action.w_a_t) rc = tail_fold4(s, *tf);
    if (rc != SF_ERR_UNSUPPORTED) return rc;
    if (s.paired) return tail_paired(s);
    if (s.query_only) return tail_query_only(s);
    return tail_plain(s);
}

static int decoder_tail_i(const sf_decoder_w* w, const sf_cands* U, int B, int H, int D, int L,
                          const float* u_prev, const float* h0, const float* c0, const float* ctx,
                          const uint8_t* ctx_mask, const int32_t* ctx_row, const sf_decoder_tape* tp,
                          const sf_follower_glue* glue, const sf_dropout* drop, uint32_t step_id,
                          const sf_pano* X_next, const sf_decoder_tape* tn, void* ws, size_t ws_bytes,
                          sf_stream stream, const TextFold* tf = nullptr, GateStep* gate = nullptr) {
    SF_CHECK_ARG(w && U && h0 && c0 && ctx && tp && B > 0 && L > 0 && (!glue || glue_ok(U, glue)) &&
                 (!X_next || tn));
    TailStep s{};
    s.gate = gate;
    s.w = w; s.us = cands(U); s.B = B; s.H = H; s.D = D; s.L = L; s.F = s.us.IMG + s.us.LOC;
    s.tp = tp; s.tn = tn; s.glue = glue;
    s.ctx = ctx; s.ctx_mask = ctx_mask; s.ctx_row = ctx_row;
    s.ar = arena(ws, ws_bytes);
    s.st = S(stream);
    s.d_h = make_dropout(drop, 2 * step_id + 1, 2);
    s.dn_in = make_dropout(drop, 2 * (step_id + 1), 2);
    s.has_xn = X_next != nullptr;
    if (X_next) s.xn = pano(X_next);
    s.paired = X_next && w->visual.w_v_t;
    s.query_only = !X_next && tn && w->visual.w_v_t;      // (tail_query_only)
    s.last_step = !X_next && !tn;              // (nothing of a next step to prepare: the text chain alone)
    const Dropout d_in = make_dropout(drop, 2 * step_id, 2);
    if (u_prev) TRY(dropout_copy(u_prev, s.F, B, s.F, tp->xin, 2 * s.F, d_in, 0, s.st));
    // (with a gate-space row of the action half: the product over [f | h0] alone, K = F + H, the row added by the cell)
    const float* xg = gate && !u_prev ? gate->xg_in : nullptr;
    TRY(lstm_fwd_i(&w->lstm, B, 2 * s.F, H, tp->xin, 2 * s.F, h0, c0, tp->h1, tp->c1, tp->gates,
                   tp->cat2 + H, 2 * H, s.d_h, s.ar, s.st, xg, s.F));
    if (xg) g_gate_steps.fetch_add(1, std::memory_order_relaxed);
    return tail_dispatch(s, tf);
}

// tail(t) WITHOUT the head of step t+1 (that runs on another stream): LSTM cell, then -- after
// publishing "h1 of this step is complete" -- the text attention and scoring chain, unpaired.
static int decoder_tail_split_i(const sf_decoder_w* w, const sf_cands* U, int B, int H, int D, int L,
                                const float* h0, const float* c0, const float* ctx, const uint8_t* ctx_mask,
                                const sf_decoder_tape* tp, const sf_follower_glue* glue, const sf_dropout* drop,
                                uint32_t step_id, unsigned* flag_h1, unsigned flag_value, void* ws,
                                size_t ws_bytes, unsigned* tickets, hipStream_t st) {
    SF_CHECK_ARG(w && U && h0 && c0 && ctx && tp && glue && glue_ok(U, glue));
    const size_t n = ws_bytes / 4;
    Arena ar{(float*)ws, n, 0, tickets};
    const CandSrc us = cands(U);
    const int F = us.IMG + us.LOC;
    const Dropout d_h = make_dropout(drop, 2 * step_id + 1, 2);
    TRY(lstm_fwd_i(&w->lstm, B, 2 * F, H, tp->xin, 2 * F, h0, c0, tp->h1, tp->c1, tp->gates, tp->cat2 + H, 2 * H,
                   d_h, ar, st));
    if (flag_h1) TRY(flag_set(flag_h1, flag_value, st));
    TRY(softdot_fwd_i(&w->text, B, L, H, nullptr, 0, ctx, ctx_mask, tp->h_tilde, tp->alpha, tp->cat2, tp->t_text,
                      ar, st, nullptr));
    return scoring_fwd_i(&w->action, us, B, H, D, tp->h_tilde, tp->logit, tp->t_a, tp->wt, tp->r, ar, st, glue);
}

int sf_attn_decoder_attend_fwd(const sf_pano* X, int B, const sf_decoder_tape* tp, const sf_dropout* drop,
                               uint32_t step_id, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(X && tp && tp->q && tp->xin && tp->alpha_v && B > 0);
    Arena ar = arena(ws, ws_bytes);
    const PanoSrc xs = pano(X);
    const int F = xs.IMG + xs.LOC;
    float* part = B <= 1024 ? ar.take(visual_attn_split_floats(B, F)) : nullptr;
    return visual_attn(0, xs, B, tp->q, F, tp->alpha_v, tp->xin + F, 2 * F, make_dropout(drop, 2 * step_id, 2), F,
                       S(stream), part, part ? ar.tickets() : nullptr);
}

int sf_attn_decoder_tail_fwd(const sf_decoder_w* w, const sf_cands* U, int B, int H, int D, int L,
                             const float* u_prev, const float* h0, const float* c0,
                             const float* ctx, const uint8_t* ctx_mask, const int32_t* ctx_row,
                             const sf_decoder_tape* tp, const sf_follower_glue* glue,
                             const sf_dropout* drop, uint32_t step_id, const sf_pano* X_next,
                             const sf_decoder_tape* tn, void* ws, size_t ws_bytes,
                             sf_stream stream) {
    SF_ENTER();
    return decoder_tail_i(w, U, B, H, D, L, u_prev, h0, c0, ctx, ctx_mask, ctx_row, tp, glue, drop,
                          step_id, X_next, tn, ws, ws_bytes, stream);
}

// ---- a6 AttnDecoderLSTM.forward (model.py:377-397) -------------------------------------------------
int sf_attn_decoder_fwd(const sf_decoder_w* w, const sf_pano* X, const sf_cands* U, int B, int H,
                        int D, int L, const float* u_prev, const float* h0, const float* c0,
                        const float* ctx, const uint8_t* ctx_mask, const int32_t* ctx_row,
                        const sf_decoder_tape* tp, const sf_follower_glue* glue,
                        const sf_dropout* drop, uint32_t step_id,
                        void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && X && U && h0 && c0 && ctx && tp && B > 0 && L > 0 && (!glue || glue_ok(U, glue)));
    // model.py:389  feature, alpha_v = visual_attention(h_0, X)  -> straight into xin[:, F:2F]: head(t);
    // model.py:391-396  drop(cat(u_prev, feature)), LSTMCell, text attention, action logits: the plain tail(t)
    TRY(decoder_head_a(w, X, B, H, D, h0, tp, drop, step_id, arena(ws, ws_bytes), stream));
    return decoder_tail_i(w, U, B, H, D, L, u_prev, h0, c0, ctx, ctx_mask, ctx_row, tp, glue, drop, step_id, nullptr,
                          nullptr, ws, ws_bytes, stream);
}

int sf_decoder_fold_build(const sf_decoder_w* w, int H, int D, int F, float* m_v, float* c_v,
                          float* m_a, float* c_a, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && m_v && c_v && m_a && c_a && w->visual.w_v_t && w->visual.w_h_t &&
                 w->action.w_a_t && w->action.w_h_t && F % 4 == 0 && D % 4 == 0 && H % 4 == 0);
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    float* wa_s = ar.take((size_t)F * D);      // W_a^T with columns scaled by w_out
    float* wo_ba = ar.take(D);                 // w_out * b_a
    float* wo_bh = ar.take(D);                 // w_out * b_h
    NEED(wa_s && wo_ba && wo_bh);
    // visual: M_v = W_v^T W_h  ([F,D] x [D,H]),  c_v = W_v^T b_h
    TRY(linear_plain(w->visual.w_v_t, D, w->visual.w_h_t, D, nullptr, F, H, D, EPI_NONE, m_v, H, ar, st));
    TRY(linear_plain(w->visual.b_h, D, w->visual.w_v_t, D, nullptr, 1, F, D, EPI_NONE, c_v, F, ar, st));
    // scoring
    TRY(scale_cols(w->action.w_a_t, D, w->action.w_out, F, D, wa_s, D, st));
    TRY(scale_cols(w->action.b_a, D, w->action.w_out, 1, D, wo_ba, D, st));
    TRY(scale_cols(w->action.b_h, D, w->action.w_out, 1, D, wo_bh, D, st));
    TRY(fill(m_a + (size_t)F * H, (size_t)4 * H, 0.f, st));
    TRY(fill(c_a + F, 4, 0.f, st));
    TRY(linear_plain(wa_s, D, w->action.w_h_t, D, nullptr, F, H, D, EPI_NONE, m_a, H, ar, st));
    TRY(linear_plain(wo_ba, D, w->action.w_h_t, D, nullptr, 1, H, D, EPI_NONE, m_a + (size_t)F * H, H, ar, st));
    TRY(linear_plain(wo_bh, D, w->action.w_a_t, D, nullptr, 1, F, D, EPI_NONE, c_a, F + 4, ar, st));
    return linear_plain(wo_bh, D, w->action.b_a, D, w->action.b_out, 1, 1, D, EPI_NONE, c_a + F, 4, ar, st);
}

// The backward of one decode step is two chains that only meet at the LSTM pointwise backward:
//   head: scoring -> h~ -> text attention  =>  dh1d (the attention path's share of d h1), and the dY
//         operands of that half; needs only the forward tape and d(logit) of ITS step;
//   tail: LSTM cell -> input gradient -> visual attention  =>  dh0, dc0; needs dh1 / dc1 of step t+1.
// So head(t-1) can run while tail(t) does (sf_follower_episode_bwd puts the heads on a side stream).
static int decoder_bwd_head_i(const sf_decoder_w* w, const sf_decoder_g* g, const sf_cands* U, int B,
                              int H, int D, int L, const float* ctx, const sf_decoder_tape* tp,
                              const sf_decoder_gtape* gt, const float* dlogit, float* dh1d, float* dctx,
                              Arena ar, hipStream_t st, const CeSrc* ce) {
    float* dht = ar.take((size_t)B * H);       // d h_tilde
    NEED(dht && dh1d);
    // with a gradient tape the scoring backward writes d(pre-tanh) straight into gt->dpre
    bool dpre_ready = false;
    float* dht_out = gt ? gt->dpre : dht;
    TRY(scoring_bwd_i(&w->action, g ? &g->action : nullptr, cands(U), B, H, D, tp->h_tilde, tp->t_a,
                      tp->wt, dlogit, dht_out, ar, st, gt, gt ? tp->h_tilde : nullptr, &dpre_ready, ce));
    if (gt && !dpre_ready) {      // not fused: dht_out holds d h~; keep it apart from gt->dpre
        TRY(add2(dht_out, H, nullptr, 0, B, H, dht, H, st));
        dht_out = dht;
    }
    return softdot_bwd_i(&w->text, g ? &g->text : nullptr, B, L, H, ctx, tp->alpha, tp->cat2, tp->t_text,
                         tp->h_tilde, dht_out, dh1d, H, dctx, ar, st, gt ? gt->dpre : nullptr,
                         gt ? gt->dt_text : nullptr, dpre_ready, gt ? gt->dcat2 : nullptr,
                         gt ? gt->ds : nullptr);
}

static int decoder_bwd_tail_i(const sf_decoder_w* w, const sf_decoder_g* g, const sf_pano* X, int B,
                              int H, int D, const float* h0, const float* c0,
                              const sf_decoder_tape* tp, const sf_decoder_gtape* gt, const float* dh1,
                              const float* dh1d, const float* dc1, float* dh0, float* dc0,
                              const sf_dropout* drop, uint32_t step_id, Arena ar, hipStream_t st) {
    const PanoSrc xs = pano(X);
    const int F = xs.IMG + xs.LOC;
    const Dropout d_in = make_dropout(drop, 2 * step_id, 2), d_h = make_dropout(drop, 2 * step_id + 1, 2);
    float* dxin = ar.take((size_t)B * 2 * F);  // d LSTM input
    NEED(dxin);
    SmallPlan dh0_plan;
    bool dh0_deferred = false;
    const float* df_slabs = nullptr;
    int df_ks = 0;
    // (the dropout between h1 and the text attention is undone inside the LSTM pointwise backward)
    TRY(lstm_bwd_i(&w->lstm, g ? &g->lstm : nullptr, B, 2 * F, H, tp->xin, 2 * F, h0, c0, tp->c1,
                   tp->gates, dh1, dh1d, dc1, dxin, 2 * F, dh0, dc0, ar, st,
                   gt ? gt->dgates : nullptr, F, &d_h,   // u_prev is detached (follower.py:502): only
                   &dh0_plan, &dh0_deferred,            // the feature half of d(LSTM input) is needed
                   &df_slabs, &df_ks));
    // dh0 = dgates W_hh rides beside the visual-attention backward (both only need the LSTM backward); the feature
    // half of d(LSTM input) reaches it as the K-split slabs of its product (no reduce launch in between)
    if (df_ks >= 1)
        return visual_bwd_i(&w->visual, g ? &g->visual : nullptr, xs, B, H, D, h0, tp->alpha_v, tp->t_v,
                            df_slabs, F, d_in, F, dh0, ar, st, gt ? gt->dq : nullptr,
                            gt ? gt->dt_v : nullptr, dh0_deferred ? &dh0_plan : nullptr, df_ks, (long)B * F);
    return visual_bwd_i(&w->visual, g ? &g->visual : nullptr, xs, B, H, D, h0, tp->alpha_v, tp->t_v,
                        dxin + F, 2 * F, d_in, F, dh0, ar, st, gt ? gt->dq : nullptr,
                        gt ? gt->dt_v : nullptr, dh0_deferred ? &dh0_plan : nullptr);
}

static int decoder_bwd_i(const sf_decoder_w* w, const sf_decoder_g* g, const sf_pano* X,
                         const sf_cands* U, int B, int H, int D, int L, const float* h0,
                         const float* c0, const float* ctx, const sf_decoder_tape* tp,
                         const sf_decoder_gtape* gt, const float* dlogit, const float* dh1,
                         const float* dc1, float* dh0, float* dc0, float* dctx,
                         const sf_dropout* drop, uint32_t step_id, void* ws, size_t ws_bytes,
                         sf_stream stream, const CeSrc* ce = nullptr) {
    SF_CHECK_ARG(w && X && U && h0 && c0 && ctx && tp && dlogit && dh0 && dc0 && B > 0 && L > 0);
    Arena ar = arena(ws, ws_bytes);
    float* dh1d = ar.take((size_t)B * H);      // d dropout(h1)
    NEED(dh1d);
    TRY(decoder_bwd_head_i(w, g, U, B, H, D, L, ctx, tp, gt, dlogit, dh1d, dctx, ar, S(stream), ce));
    return decoder_bwd_tail_i(w, g, X, B, H, D, h0, c0, tp, gt, dh1, dh1d, dc1, dh0, dc0, drop, step_id,
                              ar, S(stream));
}

int sf_attn_decoder_bwd(const sf_decoder_w* w, const sf_decoder_g* g, const sf_pano* X,
                        const sf_cands* U, int B, int H, int D, int L, const float* h0,
                        const float* c0, const float* ctx, const sf_decoder_tape* tp,
                        const sf_decoder_gtape* gt, const float* dlogit, const float* dh1,
                        const float* dc1, float* dh0, float* dc0, float* dctx,
                        const sf_dropout* drop, uint32_t step_id, void* ws, size_t ws_bytes,
                        sf_stream stream) {
    SF_ENTER();
    return decoder_bwd_i(w, g, X, U, B, H, D, L, h0, c0, ctx, tp, gt, dlogit, dh1, dc1, dh0, dc0, dctx,
                         drop, step_id, ws, ws_bytes, stream);
}

// ---- a whole follower episode (follower.py:430-539 / 1001-1020) in one call ----------------------------
// Every per-step tensor of an index-form episode is a stacked [S][...] array, so the decode loop and
// its backward need no host work between steps: the host mirror makes ONE call instead of 2 S (its
// Python + ctypes cost per step was exposed as idle gaps between the short kernels of the backward).
extern "C++" {
namespace {
// events of the two-stream episode backward (created once per host thread, timing disabled)
// (keyed by device: an event belongs to the device that was current when it was created)
std::vector<hipEvent_t>& event_pool(size_t n) {
    static thread_local std::map<int, std::vector<hipEvent_t>> pools;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::vector<hipEvent_t>& pool = pools[dev];
    while (pool.size() < n) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) break;
        pool.push_back(e);
    }
    return pool;
}

struct StepView {
    sf_pano X;
    sf_cands U;
    sf_decoder_tape tp;
    sf_follower_glue glue;
};

template <class T>
inline T* adv(T* p, size_t n) { return p ? p + n : nullptr; }

StepView step_view(const sf_follower_episode* e, int t) {
    const size_t B = e->B, H = e->H, D = e->D, L = e->L, A = e->A;
    const size_t F = e->X.IMG + e->X.LOC, V = e->X.V;
    StepView v;
    v.X = e->X;
    v.X.vp = adv(e->X.vp, t * B);
    v.X.view = adv(e->X.view, t * B);
    v.X.dense = adv(e->X.dense, t * B * V * F);
    v.U = e->U;
    v.U.vp = adv(e->U.vp, t * B);
    v.U.cand_view = adv(e->U.cand_view, t * B * A);
    v.U.cand_sincos = adv(e->U.cand_sincos, t * B * A * 4);
    v.U.a_num = adv(e->U.a_num, t * B);
    v.U.dense = adv(e->U.dense, t * B * A * F);
    const sf_decoder_tape& p = e->tape;
    v.tp.t_v = adv(p.t_v, t * B * D);
    v.tp.q = adv(p.q, t * B * F);
    v.tp.alpha_v = adv(p.alpha_v, t * B * V);
    v.tp.xin = adv(p.xin, t * B * 2 * F);
    v.tp.gates = adv(p.gates, t * B * 4 * H);
    v.tp.c1 = adv(p.c1, t * B * H);
    v.tp.h1 = adv(p.h1, t * B * H);
    v.tp.cat2 = adv(p.cat2, t * B * 2 * H);
    v.tp.t_text = adv(p.t_text, t * B * H);
    v.tp.alpha = adv(p.alpha, t * B * L);
    v.tp.h_tilde = adv(p.h_tilde, t * B * H);
    v.tp.t_a = adv(p.t_a, t * B * D);
    v.tp.wt = adv(p.wt, t * B * D);
    v.tp.r = adv(p.r, t * B * F);
    v.tp.logit = adv(p.logit, t * B * A);
    v.glue = e->glue;
    v.glue.is_valid = adv(e->glue.is_valid, t * B * A);
    v.glue.target = adv(e->glue.target, t * B);
    v.glue.a_t = adv(e->glue.a_t, t * B);
    v.glue.target_used = adv(e->glue.target_used, t * B);
    v.glue.score = adv(e->glue.score, t * B);
    v.glue.ce_term = adv(e->glue.ce_term, t * B);
    v.glue.live = adv(e->glue.live, t * B);
    v.glue.u_next = adv(p.xin, (t + 1) * B * 2 * F);        // straight into the next step's LSTM input
    v.glue.ld_u_next = (int32_t)(2 * F);
    v.glue.u_drop = e->drop.p > 0.f ? &e->drop : nullptr;
    v.glue.u_drop_stream = 2 * (e->step0 + t + 1);
    v.glue.sample_stream = e->step0 + t;
    return v;
}

// step t of a device-resident environment: state slot t -> slot t + 1 of the stacked [S + 1][...] buffers
sf_nav_io nav_view(const sf_nav_io* n, const sf_follower_episode* e, int t) {
    const size_t B = e->B, A = e->A;
    sf_nav_io v = *n;
    v.row = adv(n->row, t * B);
    v.view = adv(n->view, t * B);
    v.row_next = adv(n->row_next, t * B);
    v.vp_next = adv(n->vp_next, t * B);
    v.view_next = adv(n->view_next, t * B);
    v.a_num_next = adv(n->a_num_next, t * B);
    v.cand_view_next = adv(n->cand_view_next, t * B * A);
    v.sincos_next = adv(n->sincos_next, t * B * A * 4);
    v.target_next = adv(n->target_next, t * B);
    return v;
}

sf_decoder_gtape gtape_view(const sf_decoder_gtape* g, const sf_follower_episode* e, int t) {
    const size_t B = e->B, H = e->H, D = e->D, F = e->X.IMG + e->X.LOC;
    sf_decoder_gtape v;
    v.dgates = adv(g->dgates, t * B * 4 * H);
    v.dpre = adv(g->dpre, t * B * H);
    v.dt_text = adv(g->dt_text, t * B * H);
    v.dt_v = adv(g->dt_v, t * B * D);
    v.dq = adv(g->dq, t * B * F);
    v.dwt = adv(g->dwt, t * B * D);
    v.dta = adv(g->dta, t * B * D);
    v.dr = adv(g->dr, t * B * F);
    v.dc = adv(g->dc, t * B);
    const bool defer = g->dcat2 && g->ds;
    v.dcat2 = defer ? adv(g->dcat2, t * B * 2 * H) : nullptr;
    v.ds = defer ? adv(g->ds, t * B * e->L) : nullptr;
    v.dh1d = adv(g->dh1d, t * B * H);
    return v;
}

// the state entering step t: the episode's initial one, or what step t - 1 left in its tape slot
struct StepState {
    const float *h, *c;
};
StepState state_in(const sf_follower_episode* e, int t) {
    const size_t off = (size_t)(t - 1) * e->B * e->H;
    return t == 0 ? StepState{e->h_init, e->c_init} : StepState{e->tape.h1 + off, e->tape.c1 + off};
}

// `later` waits for everything `earlier` holds so far
int order_behind(hipStream_t later, hipStream_t earlier, hipEvent_t ev) {
    return hipEventRecord(ev, earlier) == hipSuccess && hipStreamWaitEvent(later, ev, 0) == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}
// "Fork a side stream behind the main one, join it back."  Whatever leaves the scope with the fork still open -- every
// error return -- joins it here: inside a capture an unjoined fork invalidates the graph, outside one the side stream
// would keep writing workspace the caller believes free.
struct SideFork {
    hipStream_t main, side = nullptr;       // side: null while no fork is open
    hipEvent_t ev_join = nullptr;
    int fork(hipStream_t side_st, hipEvent_t ev_fork, hipEvent_t ev_back) {
        TRY(order_behind(side_st, main, ev_fork));
        side = side_st;
        ev_join = ev_back;
        return SF_OK;
    }
    int join() {
        hipStream_t from = side;
        side = nullptr;
        return order_behind(main, from, ev_join);
    }
    ~SideFork() { if (side) (void)join(); }
};
}  // namespace
}  // extern "C++"

int sf_follower_episode_fwd(const sf_decoder_w* w, const sf_follower_episode* e, void* ws,
                            size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && e && e->S > 0 && e->B > 0 && e->h_init && e->c_init && e->ctx && e->tape.xin &&
                 e->tape.h1 && e->tape.c1 && e->glue.target && e->glue.ended);
    const sf_dropout* drop = e->drop.p > 0.f ? &e->drop : nullptr;
    StepView cur = step_view(e, 0);
    // the folded text attention (ABI 9): ctx_q = ctx W_in, ctx_o = ctx W_out[:, :H]^T, once per episode
    TextFold tfold{e->ctx_q, e->ctx_o};
    const TextFold* tf = nullptr;
    if (e->ctx_q && e->ctx_o && !drop && e->S > 1 && w->text.w_in_t && w->text.w_out && w->action.w_a_t) {
        const int M = e->B * e->L, H = e->H;
        const Arena ar = arena(ws, ws_bytes);
        TRY(linear_plain(e->ctx, H, w->text.w_in_t, H, nullptr, M, H, H, EPI_NONE, e->ctx_q, H, ar, S(stream)));
        TRY(linear_plain(e->ctx, H, w->text.w_out, 2 * H, nullptr, M, H, H, EPI_NONE, e->ctx_o, H, ar, S(stream)));
        tf = &tfold;
    }
    {
        Arena ha = arena(ws, ws_bytes);
        // the projected chain's head: attention straight from h_init through the projected rows, ONE launch instead of
        // t_v', q' and the attention (same conditions as the steps: tail_proj)
        const PanoSrc x0 = pano(&cur.X);
        ProjTables pt;
        float* part = nullptr;
        bool head_done = false;
        if (tf && !e->glue.nav && e->B <= VIS_SPLIT_MAX_B && projected_for(w, cands(&cur.U), &x0, e->B, e->H, e->L, &pt) &&
            (part = ha.take(visual_attn_split_floats(e->B, x0.IMG + x0.LOC))) && ha.tickets()) {
            const int F = x0.IMG + x0.LOC;
            const int rc = visual_attn_proj(cands(&cur.U), x0, e->B, e->H, e->L, pt, e->h_init, e->H, cur.tp.alpha_v,
                                            cur.tp.xin + F, 2 * F, make_dropout(drop, 2 * e->step0, 2), F, part, ha.tickets(),
                                            S(stream));
            if (rc == SF_OK) head_done = true;
            else if (rc != SF_ERR_UNSUPPORTED) return rc;
        }
        if (!head_done)
            TRY(decoder_head_a(w, &cur.X, e->B, e->H, e->D, e->h_init, &cur.tp, drop, e->step0, ha, stream));
    }
    // A device-resident environment (sf_nav_io of step 0 in glue.nav; state buffers stacked [S + 1][...]): the
    // panorama of step t + 1 is only known once the glue of step t has chosen its action and stepped the
    // environment (inside the scoring + glue launch), so its attention cannot ride beside tail(t); its QUERY can
    // (tape_next without X_next), and the attention follows as its own launch -- the schedule the host loop of
    // FollowerEngine.rollout issues call by call, here without host work between the launches.
    const sf_nav_io* nav0 = e->glue.nav;
    if (nav0) SF_CHECK_ARG(w->visual.w_v_t);
    if (!nav0 && e->side_stream && e->side_stream != stream && e->S > 1 && !tf) {
        // Two chains, ONE fork and ONE join per episode, ordered per step by device flags
        // (flag_wait / flag_set kernels) instead of events:
        //   main:  [wait feat(t)] gate product, cell, [set h1(t)], t_text, text attention, h~, scoring + glue
        //   side:  [wait h1(t)]  t_v', q', visual attention of step t+1, [set feat(t+1)]
        hipStream_t ms = S(stream), ss = S(e->side_stream);
        std::vector<hipEvent_t>& ev = event_pool(2);
        if (ev.size() < 2) return SF_ERR_LAUNCH;
        const Arena whole = arena(ws, ws_bytes);
        if (!whole.tk) return SF_ERR_WORKSPACE;
        const size_t side_n = std::min<size_t>(whole.cap / 4, (size_t)4 << 20);
        unsigned* flag_h1 = whole.tk + PERSIST_TICKET + 48;
        unsigned* flag_ft = whole.tk + PERSIST_TICKET + 49;
        void* side_ws = (float*)ws + (whole.cap - side_n);
        const size_t main_bytes = (whole.cap - side_n) * sizeof(float);
        TRY(flag_set(flag_h1, 0u, ms));
        TRY(flag_set(flag_ft, 0u, ms));
        SideFork fk{ms};
        TRY(fk.fork(ss, ev[0], ev[1]));
        for (int t = 0; t < e->S; ++t) {
            const bool more = t + 1 < e->S;
            StepView nxt = more ? step_view(e, t + 1) : cur;
            const StepState in = state_in(e, t);
            if (t > 0) TRY(flag_wait(flag_ft, (unsigned)t, ms));
            TRY(decoder_tail_split_i(w, &cur.U, e->B, e->H, e->D, e->L, in.h, in.c, e->ctx, e->ctx_mask, &cur.tp,
                                     &cur.glue, drop, e->step0 + t, more ? flag_h1 : nullptr, (unsigned)(t + 1), ws,
                                     main_bytes, whole.tk, ms));
            if (more) {
                TRY(flag_wait(flag_h1, (unsigned)(t + 1), ss));
                Arena sar{(float*)side_ws, side_n, 0, whole.tk};
                TRY(decoder_head_a(w, &nxt.X, e->B, e->H, e->D, cur.tp.h1, &nxt.tp, drop, e->step0 + t + 1, sar, e->side_stream));
                TRY(flag_set(flag_ft, (unsigned)(t + 1), ss));
            }
            cur = nxt;
        }
        return fk.join();
    }
    // Gate-space rows (include/sf_hip.h: sf_gate_rows_build), together with the projected chain only: launch (2) of step t
    // leaves the chosen action's row in gate space in one of two [B, 4H] buffers carved off the FRONT of the workspace (the
    // ticket region at its end keeps its address), step t + 1 runs its gate product over [f | h0] and its cell adds the row.
    // Decided once, here, before the first launch; a step whose chain declines leaves `wrote` false and the step behind
    // it runs the full product on the raw row, which every chain still writes.
    float* xg_buf[2] = {nullptr, nullptr};
    sf_gate_rows gr{};
    {
        const CandSrc us0 = cands(&cur.U);
        const PanoSrc x0 = pano(&cur.X);
        const int F = us0.IMG + us0.LOC;
        const size_t row = ((size_t)e->B * 4 * e->H + 63) & ~(size_t)63;
        const Arena whole = arena(ws, ws_bytes);
        ProjTables pt;
        const void* packed[2];
        if (tf && !nav0 && !drop && e->S > 1 && e->B <= VIS_SPLIT_MAX_B && !us0.dense && !us0.half &&
            gate_rows_lookup(us0.table, &gr) && gr.key_w == w->lstm.w_ih && gr.H == e->H && gr.V == us0.V &&
            gr.IMG == us0.IMG && gr.LOC == us0.LOC && e->H % 4 == 0 && F % 4 == 0 && 2 * F + e->H > 1024 &&
            projected_for(w, us0, &x0, e->B, e->H, e->L, &pt) && !bf16_packed(w->lstm.w_ih, w->lstm.w_hh, packed) &&
            whole.tk && 2 * row <= whole.cap / 8) {
            xg_buf[0] = (float*)ws;
            xg_buf[1] = xg_buf[0] + row;
            ws = xg_buf[1] + row;
            ws_bytes -= 2 * row * sizeof(float);
        }
    }
    const float* xg_in = nullptr;
    for (int t = 0; t < e->S; ++t) {
        const bool more = t + 1 < e->S;
        StepView nxt = more ? step_view(e, t + 1) : cur;
        const sf_nav_io nv = nav0 ? nav_view(nav0, e, t) : sf_nav_io{};
        if (nav0) cur.glue.nav = &nv;
        const StepState in = state_in(e, t);
        GateStep gs{xg_in, GateRows{gr.gu, gr.gl, more ? xg_buf[t & 1] : nullptr}, false};
        TRY(decoder_tail_i(w, &cur.U, e->B, e->H, e->D, e->L, nullptr, in.h, in.c, e->ctx, e->ctx_mask,
                           nullptr, &cur.tp, &cur.glue, drop, e->step0 + t, more && !nav0 ? &nxt.X : nullptr,
                           more ? &nxt.tp : nullptr, ws, ws_bytes, stream, tf, xg_buf[0] ? &gs : nullptr));
        xg_in = gs.wrote ? gs.rows.xg_next : nullptr;
        if (nav0 && more)
            TRY(sf_attn_decoder_attend_fwd(&nxt.X, e->B, &nxt.tp, drop, e->step0 + t + 1, ws, ws_bytes, stream));
        cur = nxt;
    }
    return SF_OK;
}

int sf_follower_episode_bwd(const sf_decoder_w* w, const sf_follower_episode* e,
                            const sf_decoder_gtape* gtape, const float* gscale, float* dlogit,
                            float* dh_a, float* dc_a, float* dh_b, float* dc_b, float* dctx,
                            int* result_in_b, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && e && gtape && gscale && dlogit && dh_a && dc_a && dh_b && dc_b && result_in_b &&
                 e->S > 0 && e->B > 0);
    const sf_dropout* drop = e->drop.p > 0.f ? &e->drop : nullptr;
    sf_decoder_gtape gt_all = *gtape;          // the deferred context gradient only where it is covered
    if (!(gt_all.dcat2 && gt_all.ds && dctx && ctx_grad_supported(e->S, e->L, e->H)))
        gt_all.dcat2 = gt_all.ds = nullptr;
    gtape = &gt_all;
    const float *dh1 = nullptr, *dc1 = nullptr;       // gradient arriving from the step behind (null: the last step)
    float *dho = dh_a, *dco = dc_a, *dhn = dh_b, *dcn = dc_b;
    // Software-pipelined over two streams when the caller gives a side stream and per-step dh1d
    // storage: the heads (scoring / text-attention backward, ~45 us of small dependent launches per
    // step) run ahead on the side stream, the tails (LSTM / visual backward, ~65 us) follow on the main
    // stream, each behind the event of its own head.  The heads write only per-step tape slots and
    // their own arena region, so nothing is shared but the events.
    hipStream_t main_st = S(stream), side_st = S(e->side_stream);
    // (up to VIS_SPLIT_MAX_B rows only: above it the tails take the un-split, un-paired visual-attention backward and
    // the tails' share of the workspace -- the heads' region is split off below -- did not hold it: the call failed with
    // SF_ERR_WORKSPACE at B = 300, while B = 256 fits.  The one-stream walk gets the whole workspace.)
    const bool two = side_st && side_st != main_st && gtape->dh1d && gtape->dcat2 && gtape->ds &&
                     e->B <= VIS_SPLIT_MAX_B;
    if (two) {
        SF_CHECK_ARG(e->ctx && dctx);
        std::vector<hipEvent_t>& ev = event_pool(e->S + 1);
        if (ev.size() < (size_t)e->S + 1) return SF_ERR_LAUNCH;      // event creation failed
        const Arena whole = arena(ws, ws_bytes);
        const size_t usable = whole.cap;
        const size_t head_n = std::min<size_t>(usable / 4, (size_t)4 << 20);
        // two disjoint regions of the one workspace; both keep the real ticket region
        Arena tail_ar{(float*)ws, usable - head_n, 0, whole.tk};
        Arena head_ar{(float*)ws + (usable - head_n), head_n, 0, whole.tk};
        // (the side stream behind the caller's stream: the forward pass)
        TRY(order_behind(side_st, main_st, ev[e->S]));
        // ALL heads are issued first (they depend on nothing the tails produce), each followed by
        // its event; then the tails, each behind the event of its head.  (Measured on MI355X: work of
        // two queues overlaps only where a kernel leaves CUs unoccupied -- tools/overlap_probe.py: an
        // 0.73 ms chain of recurrent steps beside 0.87 ms of gate products takes 1.35 ms, beside
        // chip-filling library GEMMs the plain sum, stream priority changes nothing -- so the gain of
        // the second stream is the small kernels of the heads filling the gaps of the tails.)
        for (int t = e->S - 1; t >= 0; --t) {
            StepView v = step_view(e, t);
            const sf_decoder_gtape g = gtape_view(gtape, e, t);
            const CeSrc ce{v.tp.logit, v.glue.target_used, gscale + t, -1, (int)e->A};
            TRY(decoder_bwd_head_i(w, nullptr, &v.U, e->B, e->H, e->D, e->L, e->ctx, &v.tp, &g, dlogit,
                                   g.dh1d, dctx, head_ar, side_st, &ce));
            if (hipEventRecord(ev[t], side_st) != hipSuccess) return SF_ERR_LAUNCH;
        }
        // Tail t may run once head t is complete: an event per step.  Measured by wall clock ("Retired
        // experiments"): heads alone 0.93 ms, tails alone 1.14 ms, both chains in one graph 1.46 ms, as two graphs on two
        // streams 1.43 ms -- they overlap either way.
        // (rocprofv3 --kernel-trace serialises the queues: its timelines show every head before the first tail.)
        for (int t = e->S - 1; t >= 0; --t) {
            StepView v = step_view(e, t);
            const sf_decoder_gtape g = gtape_view(gtape, e, t);
            const StepState in = state_in(e, t);
            if (hipStreamWaitEvent(main_st, ev[t], 0) != hipSuccess) return SF_ERR_LAUNCH;
            TRY(decoder_bwd_tail_i(w, nullptr, &v.X, e->B, e->H, e->D, in.h, in.c, &v.tp, &g, dh1, g.dh1d, dc1,
                                   dho, dco, drop, e->step0 + t, tail_ar, main_st));
            dh1 = dho;
            dc1 = dco;
            std::swap(dho, dhn);
            std::swap(dco, dcn);
        }
    } else {
        for (int t = e->S - 1; t >= 0; --t) {
            StepView v = step_view(e, t);
            const sf_decoder_gtape g = gtape_view(gtape, e, t);
            const StepState in = state_in(e, t);
            // the cross-entropy backward (softmax - onehot, scaled by 1 / live rows of the step) is
            // formed inside the scoring backward: one dependent launch less per step
            const CeSrc ce{v.tp.logit, v.glue.target_used, gscale + t, -1, (int)e->A};
            TRY(decoder_bwd_i(w, nullptr, &v.X, &v.U, e->B, e->H, e->D, e->L, in.h, in.c, e->ctx, &v.tp, &g,
                              dlogit, dh1, dc1, dho, dco, dctx, drop, e->step0 + t, ws, ws_bytes, stream,
                              &ce));
            dh1 = dho;
            dc1 = dco;
            std::swap(dho, dhn);
            std::swap(dco, dcn);
        }
    }
    *result_in_b = (dh1 == dh_b) ? 1 : 0;
    if (gtape->dcat2 && gtape->ds && dctx)     // the deferred context gradient, once for the episode
        TRY(ctx_grad_accum(e->tape.alpha, gtape->ds, gtape->dcat2, 2 * e->H, e->tape.t_text, e->S, e->B,
                           e->L, e->H, dctx, S(stream)));
    return SF_OK;
}

// All weight gradients of S stacked decoder steps, each as ONE product of reduction depth M = S*B.
int sf_attn_decoder_wgrad(const sf_decoder_w* w, const sf_decoder_g* g, int M, int H, int D, int F,
                          const float* h0_all, const sf_decoder_tape* tp, const sf_decoder_gtape* gt,
                          void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && g && h0_all && tp && gt && M > 0);
    hipStream_t st = S(stream);
    Arena ar = arena(ws, ws_bytes);
    // LSTMCell (model.py:393): dW_ih's leading columns (whole rounds of the chip) as one large product, its narrow tail
    // with the small matrices below
    const int q_main = gemm_tn_main_columns(M, 4 * H, 2 * F);
    if (g->lstm.w_ih) TRY(gemm_tn(gt->dgates, 4 * H, tp->xin, 2 * F, M, 4 * H, q_main, g->lstm.w_ih, 2 * F, 1, st, ar.rest(), ar.rest_n()));
    // the other matrices (a few dozen output tiles each over the same M stacked rows): one grouped launch sequence
    TnJob jobs[8];
    int nj = 0;
    auto job = [&](const float* Y, int ldy, const float* X, int ldx, int P, int Q, float* out, int ldo = 0) {
        if (out) jobs[nj++] = TnJob{Y, ldy, X, ldx, M, P, Q, out, ldo ? ldo : Q, 1};
    };
    if (g->lstm.w_ih && q_main < 2 * F)
        job(gt->dgates, 4 * H, tp->xin + q_main, 2 * F, 4 * H, 2 * F - q_main, g->lstm.w_ih + q_main, 2 * F);
    job(gt->dgates, 4 * H, h0_all, H, 4 * H, H, g->lstm.w_hh);
    job(tp->t_v, D, gt->dq, F, D, F, g->visual.w_v);                     // visual attention (model.py:389)
    job(gt->dt_v, D, h0_all, H, D, H, g->visual.w_h);
    job(gt->dpre, H, tp->cat2, 2 * H, H, 2 * H, g->text.w_out);          // text attention (model.py:395)
    job(gt->dt_text, H, tp->cat2 + H, 2 * H, H, H, g->text.w_in);
    job(tp->wt, D, gt->dr, F, D, F, g->action.w_a);                      // action scoring (model.py:396)
    job(gt->dta, D, tp->h_tilde, H, D, H, g->action.w_h);
    if (nj) TRY(gemm_tn_group(jobs, nj, st, ar.rest(), ar.rest_n()));
    if (g->lstm.w_ih || g->lstm.w_hh || g->lstm.b_ih || g->lstm.b_hh)
        TRY(colsum_pair(gt->dgates, 4 * H, M, 4 * H, g->lstm.b_ih, g->lstm.b_hh, ar, st));
    if (g->visual.b_h) TRY(colsum(gt->dt_v, D, M, D, g->visual.b_h, 1, st, nullptr, ar.rest(), ar.rest_n()));
    if (g->action.b_a) TRY(dot_rows_accum(gt->dc, tp->wt, D, M, D, g->action.b_a, st));
    if (g->action.b_out) TRY(sum_accum(gt->dc, M, g->action.b_out, st));
    if (g->action.w_out) TRY(colsum_prod(gt->dwt, D, tp->t_a, D, M, D, g->action.w_out, st));
    if (g->action.b_h) TRY(colsum(gt->dta, D, M, D, g->action.b_h, 1, st, nullptr, ar.rest(), ar.rest_n()));
    return SF_OK;
}

int sf_follower_glue_fwd(const sf_cands* U, int B, float* logit, const sf_follower_glue* glue,
                         sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(U && logit && glue && B > 0 && glue_ok(U, glue));
    return follower_glue_fwd(make_glue(cands(U), B, logit, glue), S(stream));
}

int sf_follower_glue_bwd(int B, int A, const float* logit, const int64_t* target_used,
                         const float* gscale, float* dlogit, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(logit && target_used && gscale && dlogit && B > 0 && A > 0);
    return softmax_ce_bwd(B, A, A, logit, target_used, -1, gscale, dlogit, S(stream));
}

int sf_reduce_terms(const float* term, const float* live, int T, int B, float* sum_cnt,
                    sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(term && live && sum_cnt && T > 0 && B > 0);
    return reduce_terms(term, live, T, B, sum_cnt, S(stream));
}

int sf_loss_finalize(const float* sum_cnt, int T, float* loss, float* gscale, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(sum_cnt && loss && gscale && T > 0);
    return loss_finalize(sum_cnt, T, loss, gscale, S(stream));
}

// ---- a5 EncoderLSTM.forward (model.py:81-104) --------------------------------------------------------
int sf_encoder_lstm_fwd(const sf_encoder_w* w, int B, int Lpad, int T, int E, int H,
                        const int64_t* seq, const int32_t* lengths, float* ctx, float* decoder_init,
                        float* c_t, const sf_encoder_tape* tp, const sf_dropout* drop,
                        uint32_t drop_stream, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && seq && lengths && ctx && decoder_init && c_t && tp && B > 0 && T > 0 &&
                 T <= Lpad && E % 4 == 0 && H % 16 == 0);
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    const size_t BH = (size_t)B * H;
    // model.py:85  embedding, time-major so each step reads one contiguous [B,E] block (kept for the
    // backward's dW_ih; an inference call with the input-product table passes tape->emb = NULL)
    SF_CHECK_ARG(tp->emb || w->xw_table);
    if (tp->emb) TRY(embedding_tm(w->embedding, E, seq, B, Lpad, T, tp->emb, st));
    if (w->flags & SF_ENC_EMB_DROPOUT) {         // trainable embedding: model.py:86-87 drops the embedded tokens
        SF_CHECK_ARG(tp->emb && !w->xw_table);
        TRY(dropout_tm(tp->emb, T, B, E, make_dropout(drop, drop_stream ^ 0x40000000u),
                       (w->flags & SF_ENC_REVERSED) ? lengths : nullptr, st));
    }
    // input product: a row of the host's [vocab,4H] table per token, or hoisted for all steps at
    // once ([T*B,E] x [E,4H])
    if (!w->xw_table) SF_CHECK_ARG(tp->emb && tp->xg);
    if (!w->xw_table)
        TRY(linear_plain(tp->emb, E, w->lstm.w_ih, E, nullptr, T * B, 4 * H, E, EPI_NONE, tp->xg,
                         4 * H, ar, st));
    // (SF_ENC_RAW_STATE: ctx is handed over raw as well -- the caller drops the assembled [forward | reverse] rows)
    const Dropout dctx = (w->flags & SF_ENC_RAW_STATE) ? make_dropout(nullptr, 0) : make_dropout(drop, drop_stream);
    // all T steps as ONE persistent launch (sf_persist.hip) where it applies; bit-identical results
    bool persistent = false;
    if (w->xw_table && !(w->flags & SF_ENC_PER_STEP) && encoder_persistent_supported(B, H, T)) {
        Arena pa = ar;
        float* xchg = pa.take(encoder_persistent_xchg_floats(H));
        if (xchg && ar.tickets()) {
            TRY(encoder_persistent(w->lstm.w_hh, w->lstm.b_ih, w->lstm.b_hh, w->xw_table, seq, Lpad, lengths, B,
                                   H, T, tp->gates, tp->hs, tp->cs, ctx, dctx, xchg,
                                   ar.tickets() + PERSIST_TICKET, st, c_t));
            persistent = true;
        }
    }
    if (!persistent) {
        TRY(fill(tp->hs, BH, 0.f, st));   // model.py:67-79 init_state
        TRY(fill(tp->cs, BH, 0.f, st));
    }
    for (int t = 0; t < T && !persistent; ++t) {
        // one fused launch per time step: h_t W_hh^T on the matrix cores + gates + cell update
        LstmStepArgs f{};
        f.h0 = tp->hs + t * BH; f.w_hh = w->lstm.w_hh; f.x = nullptr; f.xg = tp->xg + (size_t)t * B * 4 * H;
        if (w->xw_table) {                       // token lookup: seq is [B, Lpad], step t = column t
            f.xg = w->xw_table;
            f.xg_index = seq + t;
            f.xg_index_ld = Lpad;
        }
        f.b_ih = w->lstm.b_ih; f.b_hh = w->lstm.b_hh; f.B = B; f.H = H;
        LstmPwFwd& p = f.pw;
        p.c0 = tp->cs + t * BH; p.h0 = tp->hs + t * BH; p.B = B; p.H = H;
        p.gates = tp->gates ? tp->gates + (size_t)t * B * 4 * H : nullptr;
        p.h1 = tp->hs + (t + 1) * BH; p.c1 = tp->cs + (t + 1) * BH;
        p.h1_drop = nullptr; p.drop = make_dropout(nullptr, 0);
        p.lengths = lengths; p.t = t; p.ctx_out = ctx; p.ld_ctx = T * H; p.ctx_drop = dctx;
        TRY(lstm_step_fused(f, st));
    }
    // model.py:96-99  decoder_init = tanh(encoder2decoder(h_T)); c_T raw
    if (w->flags & SF_ENC_RAW_STATE)               // one direction of a bidirectional encoder: the raw h_T
        TRY(add2(tp->hs + T * BH, H, nullptr, 0, B, H, decoder_init, H, st));
    else
        TRY(linear_plain(tp->hs + T * BH, H, w->w_e2d, H, w->b_e2d, B, H, H, EPI_TANH, decoder_init, H,
                         ar, st));
    if (persistent) return SF_OK;                 // (the persistent launch wrote c_T itself)
    return add2(tp->cs + T * BH, H, nullptr, 0, B, H, c_t, H, st);
}

int sf_encoder_lstm_bwd(const sf_encoder_w* w, const sf_encoder_g* g, int B, int T, int E, int H,
                        const int32_t* lengths, const float* decoder_init, const float* dctx,
                        const float* d_init, const float* d_ct, const sf_encoder_tape* tp,
                        const sf_dropout* drop, uint32_t drop_stream, void* ws, size_t ws_bytes,
                        sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && lengths && decoder_init && tp && B > 0 && T > 0);
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    const size_t BH = (size_t)B * H, BG = (size_t)B * 4 * H;
    float* dh = ar.take(BH);        // gradient wrt h after step t
    float* dc = ar.take(BH);
    float* dcn = ar.take(BH);
    float* dctx_t = ar.take(BH);
    float* dpass = ar.take(BH);
    float* dpre = ar.take(BH);
    NEED(dh && dc && dcn && dctx_t && dpass && dpre);
    // through decoder_init = tanh(W h_T + b)
    if (d_init && (w->flags & SF_ENC_RAW_STATE)) {
        TRY(add2(d_init, H, nullptr, 0, B, H, dh, H, st));          // gradient wrt the raw h_T
    } else if (d_init) {
        TRY(tanh_bwd(decoder_init, H, d_init, H, B, H, dpre, H, st));
        TRY(data_grad(dpre, H, w->w_e2d, w->w_e2d_t, B, H, H, dh, H, 0, ar, st));
        if (g && g->w_e2d) TRY(gemm_tn(dpre, H, tp->hs + T * BH, H, B, H, H, g->w_e2d, H, 1, st, ar.rest(), ar.rest_n()));
        if (g && g->b_e2d) TRY(colsum(dpre, H, B, H, g->b_e2d, 1, st, nullptr, ar.rest(), ar.rest_n()));
    } else {
        TRY(fill(dh, BH, 0.f, st));
    }
    TRY(add2(d_ct, H, nullptr, 0, B, H, dc, H, st));
    const Dropout dd = (w->flags & SF_ENC_RAW_STATE) ? make_dropout(nullptr, 0) : make_dropout(drop, drop_stream);
    // dgates for step t overwrite tp->xg[t] (the hoisted product is dead after the forward)
    bool persistent = false;
    if (!(w->flags & SF_ENC_PER_STEP) && encoder_persistent_supported(B, H, T) && ar.tickets()) {
        // ALL T backward steps as one persistent launch (sf_persist.hip)
        Arena pa = ar;
        float* xchg = pa.take(encoder_bwd_persistent_xchg_floats());
        if (xchg) {
            TRY(encoder_bwd_persistent(w->lstm.w_hh, lengths, B, H, T, tp->gates, tp->cs, dctx, dd, dh, dc, tp->xg,
                                       xchg, ar.tickets() + PERSIST_TICKET, st));
            persistent = true;
        }
    }
    if (persistent) {
    } else if (w->lstm.w_hh_t && H % 16 == 0 && H <= 512) {
        // ONE launch per step: dh_{t+1} = pass + dgates_{t+1} W_hh on the matrix cores and the cell
        // backward of step t on the same tile (lstm_bwd_step_fused_kernel)
        float* dh_b = dpass;                              // ping-pong partners of dh / dc
        for (int t = T - 1; t >= 0; --t) {
            LstmBwdStepArgs f{};
            f.dgates_next = t + 1 < T ? tp->xg + (size_t)(t + 1) * BG : nullptr;
            f.w_hh_t = w->lstm.w_hh_t;
            f.dh_in = dh; f.dc_in = dc;
            f.gates = tp->gates + t * BG; f.c0 = tp->cs + t * BH; f.c1 = tp->cs + (t + 1) * BH;
            f.dctx = dctx; f.T = T; f.t = t; f.ctx_drop = dd; f.lengths = lengths; f.B = B; f.H = H;
            f.dgates = tp->xg + t * BG; f.dc_out = dcn; f.dh_out = dh_b;
            TRY(lstm_bwd_step_fused(f, st));
            std::swap(dc, dcn);
            std::swap(dh, dh_b);
        }
    } else
    for (int t = T - 1; t >= 0; --t) {
        // two dependent launches per step: the cell backward reads dctx[:, t, :] itself and leaves
        // the pass-through of dead rows IN dh (element-wise in place), then dh += dgates W_hh
        LstmPwBwd p{};
        p.gates = tp->gates + t * BG; p.c0 = tp->cs + t * BH; p.c1 = tp->cs + (t + 1) * BH;
        p.dh1 = dh; p.dh1_b = nullptr; p.dc1 = dc; p.B = B; p.H = H;
        p.dgates = tp->xg + t * BG; p.dc0 = dcn; p.lengths = lengths; p.t = t; p.dh0_pass = dh;
        p.dctx = dctx; p.T = T; p.ctx_drop = dd;
        TRY(lstm_pointwise_bwd(p, st));
        TRY(data_grad(tp->xg + t * BG, 4 * H, w->lstm.w_hh, w->lstm.w_hh_t, B, 4 * H, H, dh, H, 1, ar, st));
        std::swap(dc, dcn);
    }
    if (g) {
        // all time steps in one product each: reduction depth T*B
        if (g->lstm.w_hh) TRY(gemm_tn(tp->xg, 4 * H, tp->hs, H, T * B, 4 * H, H, g->lstm.w_hh, H, 1, st, ar.rest(), ar.rest_n()));
        if (g->lstm.w_ih) TRY(gemm_tn(tp->xg, 4 * H, tp->emb, E, T * B, 4 * H, E, g->lstm.w_ih, E, 1, st, ar.rest(), ar.rest_n()));
        TRY(colsum_pair(tp->xg, 4 * H, T * B, 4 * H, g->lstm.b_ih, g->lstm.b_hh, ar, st));
        if (g->embedding) {
            // trainable embedding (model.py:57-60): d emb = dgates W_ih for all steps at once, through the dropout of
            // the embedded tokens, scattered into the rows of their tokens
            SF_CHECK_ARG(g->seq && g->Lpad >= T);
            Arena ea = ar;
            float* demb = ea.take((size_t)T * B * E);
            NEED(demb);
            TRY(data_grad(tp->xg, 4 * H, w->lstm.w_ih, w->lstm.w_ih_t, T * B, 4 * H, E, demb, E, 0, ea, st));
            const Dropout de = (w->flags & SF_ENC_EMB_DROPOUT) ? make_dropout(drop, drop_stream ^ 0x40000000u)
                                                               : make_dropout(nullptr, 0);
            TRY(embedding_bwd(demb, E, g->seq, g->Lpad, T, B, E, g->padding_idx, de,
                              (w->flags & SF_ENC_REVERSED) ? lengths : nullptr, g->embedding, st));
        }
    }
    return SF_OK;
}

// ---- a5 bidirectional EncoderLSTM (model.py:47-66, 81-104 with bidirectional=True) -------------------------------
namespace {
EncDir enc_dir(const sf_encoder_w* w, const sf_encoder_tape* tp) {
    return EncDir{w->lstm.w_hh, w->lstm.b_ih, w->lstm.b_hh, w->xw_table, tp->gates, tp->hs, tp->cs, tp->xg};
}
bool bi_persistent(const sf_encoder_w* f, const sf_encoder_w* r, int B, int H, int T) {
    return f->xw_table && r->xw_table && !(f->flags & SF_ENC_PER_STEP) && encoder_bi_persistent_supported(B, H, T);
}
// a nested entry-point call on what is left of the arena (the ticket region stays where it is)
inline size_t nested_bytes(const Arena& a) { return (a.rest_n() + SYNC_WORDS) * 4; }
}  // namespace

int sf_encoder_bilstm_fwd(const sf_encoder_w* fwd, const sf_encoder_w* rev, const float* w_e2d, const float* b_e2d,
                          const float* w_e2d_t, int B, int Lpad, int T, int E, int H, const int64_t* seq,
                          const int32_t* lengths, float* ctx, float* decoder_init, float* c_t,
                          const sf_encoder_tape* tf, const sf_encoder_tape* tr, const sf_dropout* drop,
                          uint32_t drop_stream, int32_t* path, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    (void)w_e2d_t;
    SF_CHECK_ARG(fwd && rev && w_e2d && seq && lengths && ctx && decoder_init && c_t && tf && tr && B > 0 && T > 0 &&
                 T <= Lpad && E % 4 == 0 && H % 16 == 0 && tf->hs && tf->cs && tr->hs && tr->cs);
    SF_CHECK_ARG((tf->emb || fwd->xw_table) && (tr->emb || rev->xw_table));
    if (path) *path = 0;
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    const size_t BH = (size_t)B * H;
    float* h_out = ar.take(2 * BH);                       // [h_reverse ; h_forward]
    NEED(h_out);
    if (bi_persistent(fwd, rev, B, H, T) && ar.tickets()) {
        Arena pa = ar;
        float* xchg = pa.take(encoder_bi_persistent_xchg_floats(H));
        int64_t* seq_rev = tr->emb ? reinterpret_cast<int64_t*>(pa.take((size_t)2 * B * Lpad)) : nullptr;
        if (xchg && (seq_rev || !tr->emb)) {
            // the embedded tokens of both directions, each in its step order (kept for dW_ih)
            if (tf->emb) TRY(embedding_tm(fwd->embedding, E, seq, B, Lpad, T, tf->emb, st));
            if (tr->emb) {
                TRY(reverse_tokens(seq, Lpad, lengths, B, seq_rev, st));
                TRY(embedding_tm(rev->embedding, E, seq_rev, B, Lpad, T, tr->emb, st));
            }
            TRY(encoder_bi_persistent(enc_dir(fwd, tf), enc_dir(rev, tr), seq, Lpad, lengths, B, H, T, ctx,
                                      make_dropout(drop, drop_stream), h_out, c_t, xchg, ar.tickets() + PERSIST_TICKET,
                                      st));
            if (path) *path = 1;
            return linear_plain(h_out, 2 * H, w_e2d, 2 * H, b_e2d, B, 2 * H, 2 * H, EPI_TANH, decoder_init, 2 * H,
                                pa, st);
        }
    }
    // the per-step kernels: each direction through sf_encoder_lstm_fwd (raw state, undropped ctx), then the assembly
    int64_t* seq_rev = reinterpret_cast<int64_t*>(ar.take((size_t)2 * B * Lpad));
    float* ctx_f = ar.take((size_t)B * T * H);
    float* ctx_r = ar.take((size_t)B * T * H);
    float* st4 = ar.take(4 * BH);                         // raw h_T and c_T of both directions
    NEED(seq_rev && ctx_f && ctx_r && st4);
    TRY(reverse_tokens(seq, Lpad, lengths, B, seq_rev, st));
    sf_encoder_w wf = *fwd, wr = *rev;
    wf.flags |= SF_ENC_RAW_STATE;
    wr.flags |= SF_ENC_RAW_STATE | SF_ENC_REVERSED;
    TRY(sf_encoder_lstm_fwd(&wf, B, Lpad, T, E, H, seq, lengths, ctx_f, st4, st4 + BH, tf, drop, drop_stream,
                            ar.rest(), nested_bytes(ar), stream));
    TRY(sf_encoder_lstm_fwd(&wr, B, Lpad, T, E, H, seq_rev, lengths, ctx_r, st4 + 2 * BH, st4 + 3 * BH, tr, drop,
                            drop_stream, ar.rest(), nested_bytes(ar), stream));
    TRY(bi_assemble(ctx_f, ctx_r, lengths, B, T, H, make_dropout(drop, drop_stream), ctx, st));
    TRY(add2(st4 + 2 * BH, H, nullptr, 0, B, H, h_out, 2 * H, st));         // model.py:93-94: [-1] (reverse) first
    TRY(add2(st4, H, nullptr, 0, B, H, h_out + H, 2 * H, st));
    TRY(add2(st4 + 3 * BH, H, nullptr, 0, B, H, c_t, 2 * H, st));
    TRY(add2(st4 + BH, H, nullptr, 0, B, H, c_t + H, 2 * H, st));
    return linear_plain(h_out, 2 * H, w_e2d, 2 * H, b_e2d, B, 2 * H, 2 * H, EPI_TANH, decoder_init, 2 * H, ar, st);
}

int sf_encoder_bilstm_bwd(const sf_encoder_w* fwd, const sf_encoder_w* rev, const float* w_e2d, const float* w_e2d_t,
                          const sf_encoder_g* g_fwd, const sf_encoder_g* g_rev, float* g_w_e2d, float* g_b_e2d, int B,
                          int T, int E, int H, const int32_t* lengths, const float* decoder_init, const float* dctx,
                          const float* d_init, const float* d_ct, const sf_encoder_tape* tf,
                          const sf_encoder_tape* tr, const sf_dropout* drop, uint32_t drop_stream, int32_t* path,
                          void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(fwd && rev && w_e2d && lengths && decoder_init && tf && tr && B > 0 && T > 0 && E % 4 == 0 &&
                 H % 16 == 0 && tf->gates && tf->cs && tf->hs && tf->xg && tr->gates && tr->cs && tr->hs && tr->xg);
    if (path) *path = 0;
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    const size_t BH = (size_t)B * H;
    // through decoder_init = tanh(encoder2decoder([h_r ; h_f])): dh [B,2H] = gradient wrt the raw [h_r ; h_f]
    float* dh = ar.take(2 * BH);
    float* dpre = ar.take(2 * BH);
    NEED(dh && dpre);
    if (d_init) {
        TRY(tanh_bwd(decoder_init, 2 * H, d_init, 2 * H, B, 2 * H, dpre, 2 * H, st));
        TRY(data_grad(dpre, 2 * H, w_e2d, w_e2d_t, B, 2 * H, 2 * H, dh, 2 * H, 0, ar, st));
        if (g_w_e2d) {
            TRY(gemm_tn(dpre, 2 * H, tr->hs + T * BH, H, B, 2 * H, H, g_w_e2d, 2 * H, 1, st, ar.rest(), ar.rest_n()));
            TRY(gemm_tn(dpre, 2 * H, tf->hs + T * BH, H, B, 2 * H, H, g_w_e2d + H, 2 * H, 1, st, ar.rest(), ar.rest_n()));
        }
        if (g_b_e2d) TRY(colsum(dpre, 2 * H, B, 2 * H, g_b_e2d, 1, st, nullptr, ar.rest(), ar.rest_n()));
    }
    const bool emb_grad = (g_fwd && g_fwd->embedding) || (g_rev && g_rev->embedding);
    if (bi_persistent(fwd, rev, B, H, T) && !emb_grad && ar.tickets()) {
        Arena pa = ar;
        float* xchg = pa.take(encoder_bi_bwd_persistent_xchg_floats());
        if (xchg) {
            TRY(encoder_bi_bwd_persistent(enc_dir(fwd, tf), enc_dir(rev, tr), lengths, B, H, T, dctx,
                                          make_dropout(drop, drop_stream), d_init ? dh : nullptr, d_ct, xchg,
                                          ar.tickets() + PERSIST_TICKET, st));
            if (path) *path = 1;
            // the weight gradients of both directions (dgates in tape->xg): one grouped sequence of many-row products
            TnJob jobs[4];
            int nj = 0;
            const sf_encoder_g* gs[2] = {g_fwd, g_rev};
            const sf_encoder_tape* ts[2] = {tf, tr};
            for (int d = 0; d < 2; ++d) {
                if (!gs[d]) continue;
                if (gs[d]->lstm.w_hh) jobs[nj++] = TnJob{ts[d]->xg, 4 * H, ts[d]->hs, H, T * B, 4 * H, H, gs[d]->lstm.w_hh, H, 1};
                if (gs[d]->lstm.w_ih) {
                    SF_CHECK_ARG(ts[d]->emb);
                    jobs[nj++] = TnJob{ts[d]->xg, 4 * H, ts[d]->emb, E, T * B, 4 * H, E, gs[d]->lstm.w_ih, E, 1};
                }
            }
            if (nj) TRY(gemm_tn_group(jobs, nj, st, pa.rest(), pa.rest_n()));
            for (int d = 0; d < 2; ++d)
                if (gs[d]) TRY(colsum_pair(ts[d]->xg, 4 * H, T * B, 4 * H, gs[d]->lstm.b_ih, gs[d]->lstm.b_hh, pa, st));
            return SF_OK;
        }
    }
    // the per-step kernels: the assembled gradients taken apart, each direction through sf_encoder_lstm_bwd (raw state)
    float* dctx_f = ar.take((size_t)B * T * H);
    float* dctx_r = ar.take((size_t)B * T * H);
    float* halves = ar.take(4 * BH);                      // dh_f, dh_r, dc_f, dc_r
    int64_t* seq_rev = reinterpret_cast<int64_t*>(ar.take((size_t)2 * B * T));
    NEED(dctx_f && dctx_r && halves && seq_rev);
    if (dctx) TRY(bi_split(dctx, lengths, B, T, H, make_dropout(drop, drop_stream), dctx_f, dctx_r, st));
    else {
        TRY(fill(dctx_f, (size_t)B * T * H, 0.f, st));
        TRY(fill(dctx_r, (size_t)B * T * H, 0.f, st));
    }
    if (d_init) {
        TRY(add2(dh + H, 2 * H, nullptr, 0, B, H, halves, H, st));
        TRY(add2(dh, 2 * H, nullptr, 0, B, H, halves + BH, H, st));
    }
    if (d_ct) {
        TRY(add2(d_ct + H, 2 * H, nullptr, 0, B, H, halves + 2 * BH, H, st));
        TRY(add2(d_ct, 2 * H, nullptr, 0, B, H, halves + 3 * BH, H, st));
    }
    sf_encoder_w wf = *fwd, wr = *rev;
    wf.flags |= SF_ENC_RAW_STATE;
    wr.flags |= SF_ENC_RAW_STATE | SF_ENC_REVERSED;
    sf_encoder_g gf{}, gr{};
    if (g_fwd) gf = *g_fwd;
    if (g_rev) gr = *g_rev;
    gf.w_e2d = gf.b_e2d = gr.w_e2d = gr.b_e2d = nullptr;
    if (gr.embedding) {                                   // the reverse direction's tokens in its step order
        SF_CHECK_ARG(gr.seq && gr.Lpad >= T);
        Arena sa = ar;
        int64_t* sr = reinterpret_cast<int64_t*>(sa.take((size_t)2 * B * gr.Lpad));
        NEED(sr);
        TRY(reverse_tokens(gr.seq, gr.Lpad, lengths, B, sr, st));
        gr.seq = sr;
        ar = sa;
    }
    TRY(sf_encoder_lstm_bwd(&wf, g_fwd ? &gf : nullptr, B, T, E, H, lengths, decoder_init, dctx_f,
                            d_init ? halves : nullptr, d_ct ? halves + 2 * BH : nullptr, tf, drop, drop_stream,
                            ar.rest(), nested_bytes(ar), stream));
    TRY(sf_encoder_lstm_bwd(&wr, g_rev ? &gr : nullptr, B, T, E, H, lengths, decoder_init, dctx_r,
                            d_init ? halves + BH : nullptr, d_ct ? halves + 3 * BH : nullptr, tr, drop, drop_stream,
                            ar.rest(), nested_bytes(ar), stream));
    return SF_OK;
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

// ---- a9 SpeakerDecoderLSTM.forward (model.py:497-519) -----------------------------------------------------
int sf_speaker_decoder_fwd(const sf_spk_decoder_w* w, int B, int E, int H, int Tp, int vocab,
                           const int64_t* prev_word, const float* h0, const float* c0,
                           const float* ctx, const uint8_t* ctx_mask, const int32_t* ctx_row,
                           const sf_spk_decoder_tape* tp, const sf_dropout* drop, uint32_t step_id,
                           void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && prev_word && h0 && c0 && ctx && tp && B > 0 && Tp > 0 && vocab > 0);
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    const int ldv = (vocab + 3) & ~3;
    const Dropout d_h = make_dropout(drop, 2 * step_id + 1, 2);
    if (tp->emb) TRY(embedding_rows(w->embedding, E, prev_word, B, tp->emb, st));   // :497-498
    if (w->flags & SF_SPK_EMB_DROPOUT) {          // trainable embedding: :499-500 drops the embedded word
        SF_CHECK_ARG(tp->emb && !w->xw_table);
        TRY(dropout_tm(tp->emb, 1, B, E, make_dropout(drop, 2 * step_id, 2), nullptr, st));
    }
    if (w->xw_table && H % 16 == 0 && H <= 1024) {
        // x W_ih^T is a row of the precomputed [vocab,4H] table: recurrent half only
        LstmStepArgs f{};
        f.h0 = h0; f.w_hh = w->lstm.w_hh; f.x = nullptr; f.xg = w->xw_table; f.xg_index = prev_word;
        f.b_ih = w->lstm.b_ih; f.b_hh = w->lstm.b_hh; f.B = B; f.H = H;
        LstmPwFwd& p = f.pw;
        p.c0 = c0; p.h0 = h0; p.B = B; p.H = H; p.gates = tp->gates; p.h1 = tp->h1; p.c1 = tp->c1;
        p.h1_drop = tp->cat2 + H; p.ld_h1_drop = 2 * H; p.drop = d_h; p.lengths = nullptr;
        TRY(lstm_step_fused(f, st));                                              // :515-516
    } else {
        SF_CHECK_ARG(tp->emb);
        TRY(lstm_fwd_i(&w->lstm, B, E, H, tp->emb, E, h0, c0, tp->h1, tp->c1, tp->gates,
                       tp->cat2 + H, 2 * H, d_h, ar, st));                        // :515-516
    }
    TRY(softdot_fwd_i(&w->attn, B, Tp, H, nullptr, 0, ctx, ctx_mask, tp->h_tilde, tp->alpha, tp->cat2,
                      tp->t_text, ar, st, ctx_row));                              // :517
    // (columns vocab..ldv-1 of tape->logit are padding: never read by the glue; callers slice)
    return linear_plain(tp->h_tilde, H, w->w_out, H, w->b_out, B, vocab, H, EPI_NONE, tp->logit, ldv,
                        ar, st);                                                  // :518
}

// The whole word loop of an inference pass in one persistent launch (sf_persist.hip)
int sf_speaker_decode(const sf_spk_decoder_w* w, int B, int H, int Tp, int vocab, int n_steps, int feedback,
                      int pad_idx, int eos_idx, const int64_t* targets, const float* h_init,
                      const float* c_init, const float* ctx, const uint8_t* ctx_mask, int64_t* words,
                      uint8_t* ended, float* step_scores, float* nll_term, float* live, float* logits,
                      float* alpha, float* h1_tape, float* c1_tape, const sf_sample* sample, void* ws,
                      size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && targets && h_init && c_init && ctx && words && ended && step_scores && nll_term && live &&
                 B > 0 && n_steps > 0 && Tp > 0 && feedback >= 0 && feedback <= 2 && (feedback != 2 || sample) &&
                 (!h1_tape == !c1_tape));
    if (!w->xw_table || !w->attn.w_in_t || !speaker_persistent_supported(B, H, Tp, vocab)) return SF_ERR_UNSUPPORTED;
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    float* cq = ar.take((size_t)B * Tp * H);
    float* cw = ar.take((size_t)B * Tp * H);
    float* xchg = ar.take(speaker_persistent_xchg_floats());
    NEED(cq && cw && xchg && ar.tickets());
    // cq = ctx W_in (so that ctx_l . (W_in h) = cq_l . h), cw = ctx W_c^T with W_c = linear_out[:, :H]
    TRY(linear_plain(ctx, H, w->attn.w_in_t, H, nullptr, B * Tp, H, H, EPI_NONE, cq, H, ar, st));
    TRY(linear_plain(ctx, H, w->attn.w_out, 2 * H, nullptr, B * Tp, H, H, EPI_NONE, cw, H, ar, st));
    const int ldv = (vocab + 3) & ~3;
    return speaker_persistent(w->lstm.w_hh, w->lstm.b_ih, w->lstm.b_hh, w->xw_table, w->attn.w_out, 2 * H, w->w_out,
                              w->b_out, vocab, ldv, cq, cw, ctx_mask, h_init, c_init, targets, feedback, pad_idx,
                              eos_idx, B, H, Tp, n_steps, words, step_scores, nll_term, live, logits, alpha, h1_tape,
                              c1_tape, ended, xchg, ar.tickets() + PERSIST_TICKET, st, sample);
}

// d h~ = dlogit W_out (dlogit [B,ldv] with zero padding columns): K-contiguous through decoder2action^T when the host
// keeps it (sf_spk_decoder_w.w_out_t [H,ldv]), else the strided NN kernel
static int spk_dlogit_to_dht(const sf_spk_decoder_w* w, const float* dlogit, int ldv, int B, int H, int vocab, float* dht,
                             Arena& ar, hipStream_t st) {
    if (w->w_out_t) {
        Seg sg{dlogit, ldv, w->w_out_t, ldv, ldv};
        LinearOut o{};
        o.y = dht; o.ldy = H; o.epi = EPI_NONE;
        const int rc = linear_nt(&sg, 1, B, H, o, ar.rest(), ar.rest_n(), st);
        if (rc != SF_ERR_UNSUPPORTED) return rc;
    }
    return gemm_nn_ws(dlogit, ldv, w->w_out, H, B, H, vocab, dht, H, 0, ar.rest(), ar.rest_n(), st);
}

int sf_speaker_decoder_bwd(const sf_spk_decoder_w* w, const sf_spk_decoder_g* g, int B, int E, int H,
                           int Tp, int vocab, const int64_t* prev_word, const float* h0, const float* c0, const float* ctx,
                           const sf_spk_decoder_tape* tp, const float* dlogit, const float* dh1,
                           const float* dc1, float* dh0, float* dc0, float* dctx,
                           const sf_dropout* drop, uint32_t step_id, void* ws, size_t ws_bytes,
                           sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && h0 && c0 && ctx && tp && dlogit && dh0 && dc0 && B > 0);
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    const int ldv = (vocab + 3) & ~3;
    const Dropout d_h = make_dropout(drop, 2 * step_id + 1, 2);
    float* dht = ar.take((size_t)B * H);
    float* dh1d = ar.take((size_t)B * H);
    float* dh1m = ar.take((size_t)B * H);
    NEED(dht && dh1d && dh1m);
    // dlogit [B,ldv] has zeros in its padding columns
    TRY(spk_dlogit_to_dht(w, dlogit, ldv, B, H, vocab, dht, ar, st));
    if (g && g->w_out) TRY(gemm_tn(dlogit, ldv, tp->h_tilde, H, B, vocab, H, g->w_out, H, 1, st, ar.rest(), ar.rest_n()));
    if (g && g->b_out) TRY(colsum(dlogit, ldv, B, vocab, g->b_out, 1, st, nullptr, ar.rest(), ar.rest_n()));
    TRY(softdot_bwd_i(&w->attn, g ? &g->attn : nullptr, B, Tp, H, ctx, tp->alpha, tp->cat2,
                      tp->t_text, tp->h_tilde, dht, dh1d, H, dctx, ar, st));
    TRY(dropout_copy(dh1d, H, B, H, dh1m, H, d_h, 0, st));
    // a frozen (GloVe) embedding needs no gradient wrt the LSTM input (model.py:472); a trainable one gets
    // d emb = dgates W_ih through its dropout, scattered into the rows of the previous words
    if (!(g && g->embedding))
        return lstm_bwd_i(&w->lstm, g ? &g->lstm : nullptr, B, E, H, tp->emb, E, h0, c0, tp->c1,
                          tp->gates, dh1, dh1m, dc1, nullptr, 0, dh0, dc0, ar, st);
    SF_CHECK_ARG(prev_word && tp->emb);
    float* demb = ar.take((size_t)B * E);
    NEED(demb);
    TRY(lstm_bwd_i(&w->lstm, &g->lstm, B, E, H, tp->emb, E, h0, c0, tp->c1, tp->gates, dh1, dh1m, dc1, demb, E, dh0, dc0,
                   ar, st));
    const Dropout de = (w->flags & SF_SPK_EMB_DROPOUT) ? make_dropout(drop, 2 * step_id, 2) : make_dropout(nullptr, 0);
    return embedding_bwd(demb, E, prev_word, 1, 1, B, E, -1, de, nullptr, g->embedding, st);
}

int sf_speaker_glue_fwd(int B, int vocab, int ldv, const float* logit, const int64_t* target,
                        int feedback, int pad_idx, int eos_idx, uint8_t* ended, int64_t* w_t,
                        float* score, float* nll_term, float* live, const sf_sample* sample, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(logit && target && ended && w_t && score && nll_term && live && B > 0 &&
                 vocab > 0 && ldv >= vocab && feedback >= 0 && feedback <= 2 && (feedback != 2 || sample));
    return speaker_glue_fwd(B, vocab, ldv, logit, target, feedback, pad_idx, eos_idx, ended, w_t,
                            score, nll_term, live, S(stream), sample);
}
int sf_speaker_sample_max_vocab(void) { return speaker_sample_max_vocab(); }

// ---- a8 SpeakerEncoderLSTM.forward (model.py:437-457), all path steps in one call -------------------------------------
static int speaker_encoder_fwd_i(const sf_visual_fold64* fold64, const sf_visual_w* vw, const sf_lstm_w* lw, const float* w_e2d, const float* b_e2d,
                           const sf_pano* X0, int Tp, int B, int H, int D, float* xin, float* alpha, float* t_v,
                           float* q, float* gates, float* hs, float* cs, float* ctx, const float* act_emb,
                           float* h_init, const sf_dropout* drop, uint32_t step0, void* ws, size_t ws_bytes,
                           sf_stream stream) {
    SF_CHECK_ARG(vw && lw && w_e2d && X0 && X0->vp && X0->view && Tp > 0 && B > 0 && xin && alpha && t_v && q && gates && hs &&
                 cs && h_init && (!act_emb || drop) && (!ctx || !drop));
    const int F = X0->IMG + X0->LOC, V = X0->V;
    const size_t BH = (size_t)B * H;
    for (int t = 0; t < Tp; ++t) {
        sf_pano X = *X0;
        X.vp = adv(X0->vp, (size_t)t * B);
        X.view = adv(X0->view, (size_t)t * B);
        float* x_t = xin + (size_t)t * B * 2 * F;
        // (float64 query and scores: see visual_fwd_i / csrc/sf_precise.hip; sf_debug_precise_attention(0) = fp32)
        TRY(visual_fwd_i(vw, pano(&X), B, H, D, hs + t * BH, x_t + F, 2 * F, alpha + (size_t)t * B * V,
                         t_v + (size_t)t * B * D, q + (size_t)t * B * F, make_dropout(drop, 2 * (step0 + t), 2), F,
                         arena(ws, ws_bytes), S(stream), g_precise_attention != 0, fold64));
        if (act_emb)
            TRY(dropout_copy(act_emb + (size_t)t * B * F, F, B, F, x_t, 2 * F, make_dropout(drop, 2 * (step0 + t), 2), 0,
                             S(stream)));
        TRY(sf_lstm_cell_fwd(lw, B, 2 * F, H, x_t, 2 * F, hs + t * BH, cs + t * BH, hs + (t + 1) * BH, cs + (t + 1) * BH,
                             gates + (size_t)t * B * 4 * H, ctx ? ctx + (size_t)t * H : nullptr, ctx ? Tp * H : 0, nullptr, 0,
                             ws, ws_bytes, stream));
    }
    return sf_linear_fwd(hs + Tp * BH, H, w_e2d, b_e2d, B, H, H, 1, h_init, H, ws, ws_bytes, stream);
}

int sf_speaker_encoder_fwd(const sf_visual_w* vw, const sf_lstm_w* lw, const float* w_e2d, const float* b_e2d,
                           const sf_pano* X0, int Tp, int B, int H, int D, float* xin, float* alpha, float* t_v,
                           float* q, float* gates, float* hs, float* cs, float* ctx, const float* act_emb,
                           float* h_init, const sf_dropout* drop, uint32_t step0, void* ws, size_t ws_bytes,
                           sf_stream stream) {
    SF_ENTER();
    return speaker_encoder_fwd_i(nullptr, vw, lw, w_e2d, b_e2d, X0, Tp, B, H, D, xin, alpha, t_v, q, gates, hs, cs, ctx, act_emb,
                                 h_init, drop, step0, ws, ws_bytes, stream);
}

int sf_speaker_encoder_fwd_folded(const sf_visual_fold64* fold, const sf_visual_w* vw, const sf_lstm_w* lw, const float* w_e2d,
                                  const float* b_e2d, const sf_pano* X0, int Tp, int B, int H, int D, float* xin, float* alpha,
                                  float* t_v, float* q, float* gates, float* hs, float* cs, float* ctx, const float* act_emb,
                                  float* h_init, const sf_dropout* drop, uint32_t step0, void* ws, size_t ws_bytes,
                                  sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(fold && fold->m_v && fold->c_v);
    return speaker_encoder_fwd_i(fold, vw, lw, w_e2d, b_e2d, X0, Tp, B, H, D, xin, alpha, t_v, q, gates, hs, cs, ctx, act_emb,
                                 h_init, drop, step0, ws, ws_bytes, stream);
}

int sf_visual_query_fold_f64(const sf_visual_w* w, int H, int D, int F, double* m_v, double* c_v, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && w->w_v_t && w->w_h_t && w->b_h && m_v && c_v && H > 0 && D > 0 && F > 0 && !(D & 3));
    // M_v[F,H] = W_v^T[F,D] (W_h^T[H,D])^T, c_v[1,F] = b_h[1,D] (W_v^T[F,D])^T -- both accumulated and kept in float64
    TRY(linear_f64(w->w_v_t, nullptr, D, w->w_h_t, D, nullptr, F, H, D, m_v, H, nullptr, 0, S(stream)));
    return linear_f64(w->b_h, nullptr, D, w->w_v_t, D, nullptr, 1, F, D, c_v, F, nullptr, 0, S(stream));
}

// ---- the speaker's word loop with its tape, one call each way (speaker.py:158-197 and its backward) ------------------
namespace {
sf_spk_decoder_tape spk_tape_view(const sf_spk_decoder_tape* p, int t, int B, int E, int H, int Tp, int ldv) {
    sf_spk_decoder_tape v;
    const size_t n = (size_t)t * B;
    v.emb = adv(p->emb, n * E);
    v.gates = adv(p->gates, n * 4 * H);
    v.c1 = adv(p->c1, n * H);
    v.h1 = adv(p->h1, n * H);
    v.cat2 = adv(p->cat2, n * 2 * H);
    v.t_text = adv(p->t_text, n * H);
    v.alpha = adv(p->alpha, n * Tp);
    v.h_tilde = adv(p->h_tilde, n * H);
    v.logit = adv(p->logit, n * ldv);
    return v;
}
}  // namespace

int sf_speaker_words_fwd(const sf_spk_decoder_w* w, int B, int E, int H, int Tp, int vocab, int S, int feedback,
                         int pad_idx, int eos_idx, const int64_t* targets, const float* h_init, const float* c_init,
                         const float* ctx, const uint8_t* ctx_mask, int64_t* words, uint8_t* ended, float* step_scores,
                         float* nll_term, float* live, const sf_spk_decoder_tape* tape0, const sf_dropout* drop,
                         uint32_t step0, const sf_sample* sample, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && tape0 && tape0->h1 && tape0->c1 && tape0->logit && targets && h_init && c_init && ctx && words &&
                 ended && step_scores && nll_term && live && B > 0 && S > 0 && (feedback != 2 || sample));
    const int ldv = (vocab + 3) & ~3;
    const size_t BH = (size_t)B * H;
    // with the input-product table the steps never read the embedded words: they are only kept for the backward's
    // dW_ih, so ALL S*B of them are gathered by one launch behind the loop (words [S+1,B] is complete by then)
    const bool emb_late = tape0->emb && w->xw_table && !(w->flags & SF_SPK_EMB_DROPOUT) && H % 16 == 0 && H <= 1024;
    for (int t = 0; t < S; ++t) {
        sf_spk_decoder_tape tp = spk_tape_view(tape0, t, B, E, H, Tp, ldv);
        if (emb_late) tp.emb = nullptr;
        const float* h0 = t == 0 ? h_init : tape0->h1 + (size_t)(t - 1) * BH;
        const float* c0 = t == 0 ? c_init : tape0->c1 + (size_t)(t - 1) * BH;
        TRY(sf_speaker_decoder_fwd(w, B, E, H, Tp, vocab, words + (size_t)t * B, h0, c0, ctx, ctx_mask, nullptr, &tp, drop,
                                   step0 + t, ws, ws_bytes, stream));
        sf_sample smp{};
        if (sample) {
            smp = *sample;
            smp.stream = sample->stream + (uint32_t)t;
        }
        TRY(sf_speaker_glue_fwd(B, vocab, ldv, tp.logit, targets + (size_t)t * B, feedback, pad_idx, eos_idx, ended,
                                words + (size_t)(t + 1) * B, step_scores + (size_t)t * B, nll_term + (size_t)t * B,
                                live + (size_t)t * B, sample ? &smp : nullptr, stream));
    }
    if (emb_late) TRY(embedding_rows(w->embedding, E, words, S * B, tape0->emb, (hipStream_t)stream));
    return SF_OK;
}

int sf_speaker_words_bwd(const sf_spk_decoder_w* w, const sf_spk_decoder_g* g, int B, int E, int H, int Tp, int vocab,
                         int S, int pad_idx, const int64_t* words, const int64_t* targets, const float* h_init,
                         const float* c_init, const float* ctx, const sf_spk_decoder_tape* tape0, const float* gscale,
                         float* dlogit, float* dh_a, float* dc_a, float* dh_b, float* dc_b, float* dctx,
                         int* result_in_b, const sf_dropout* drop, uint32_t step0, const sf_spk_decoder_gtape* gtape,
                         const float* h0_all, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && tape0 && tape0->h1 && tape0->c1 && tape0->logit && words && targets && h_init && c_init && ctx &&
                 gscale && (dlogit || gtape) && dh_a && dc_a && dh_b && dc_b && dctx && result_in_b && B > 0 && S > 0 &&
                 (!gtape || (gtape->dlogit && gtape->dpre && gtape->dt_text && gtape->dgates && h0_all)));
    const int ldv = (vocab + 3) & ~3;
    const size_t BH = (size_t)B * H;
    const float *dh1 = nullptr, *dc1 = nullptr;
    float *dho = dh_a, *dco = dc_a, *dhn = dh_b, *dcn = dc_b;
    hipStream_t st = (hipStream_t)stream;        // (the parameter S shadows the S() cast helper here)
    for (int t = S - 1; t >= 0; --t) {
        const sf_spk_decoder_tape tp = spk_tape_view(tape0, t, B, E, H, Tp, ldv);
        const float* h0 = t == 0 ? h_init : tape0->h1 + (size_t)(t - 1) * BH;
        const float* c0 = t == 0 ? c_init : tape0->c1 + (size_t)(t - 1) * BH;
        float* dl = gtape ? gtape->dlogit + (size_t)t * B * ldv : dlogit;
        TRY(sf_speaker_glue_bwd(B, vocab, ldv, tp.logit, targets + (size_t)t * B, pad_idx, gscale + t, dl, stream));
        if (!gtape) {
            TRY(sf_speaker_decoder_bwd(w, g, B, E, H, Tp, vocab, words + (size_t)t * B, h0, c0, ctx, &tp, dl, dh1, dc1, dho,
                                       dco, dctx, drop, step0 + t, ws, ws_bytes, stream));
        } else {
            // data gradients only; dY operands into the stacked gtape (sf_speaker_decoder_bwd with g = NULL)
            Arena ar = arena(ws, ws_bytes);
            const Dropout d_h = make_dropout(drop, 2 * (step0 + t) + 1, 2);
            float* dht = ar.take(BH);
            float* dh1d = ar.take(BH);
            float* dh1m = ar.take(BH);
            NEED(dht && dh1d && dh1m);
            TRY(spk_dlogit_to_dht(w, dl, ldv, B, H, vocab, dht, ar, st));
            TRY(softdot_bwd_i(&w->attn, nullptr, B, Tp, H, ctx, tp.alpha, tp.cat2, tp.t_text, tp.h_tilde, dht, dh1d, H, dctx,
                              ar, st, gtape->dpre + (size_t)t * BH, gtape->dt_text + (size_t)t * BH));
            // (the mask of dropout(h1) is applied to dh1d inside the LSTM pointwise backward: no copy launch)
            (void)dh1m;
            float* dgt = gtape->dgates + (size_t)t * B * 4 * H;
            if (!(g && g->embedding)) {
                TRY(lstm_bwd_i(&w->lstm, nullptr, B, E, H, tp.emb, E, h0, c0, tp.c1, tp.gates, dh1, dh1d, dc1, nullptr, 0,
                               dho, dco, ar, st, dgt, 0, &d_h));
            } else {
                SF_CHECK_ARG(tp.emb);
                float* demb = ar.take((size_t)B * E);
                NEED(demb);
                TRY(lstm_bwd_i(&w->lstm, nullptr, B, E, H, tp.emb, E, h0, c0, tp.c1, tp.gates, dh1, dh1d, dc1, demb, E, dho,
                               dco, ar, st, dgt, 0, &d_h));
                const Dropout de = (w->flags & SF_SPK_EMB_DROPOUT) ? make_dropout(drop, 2 * (step0 + t), 2)
                                                                   : make_dropout(nullptr, 0);
                TRY(embedding_bwd(demb, E, words + (size_t)t * B, 1, 1, B, E, -1, de, nullptr, g->embedding, st));
            }
        }
        dh1 = dho;
        dc1 = dco;
        std::swap(dho, dhn);
        std::swap(dco, dcn);
    }
    *result_in_b = (dh1 == dh_b) ? 1 : 0;
    if (gtape && g) {
        // every weight gradient as ONE product over the S*B stacked rows
        Arena ar = arena(ws, ws_bytes);
        const int M = S * B;
        if (g->w_out) TRY(gemm_tn(gtape->dlogit, ldv, tape0->h_tilde, H, M, vocab, H, g->w_out, H, 1, st, ar.rest(), ar.rest_n()));
        if (g->b_out) TRY(colsum(gtape->dlogit, ldv, M, vocab, g->b_out, 1, st, nullptr, ar.rest(), ar.rest_n()));
        if (g->attn.w_out) TRY(gemm_tn(gtape->dpre, H, tape0->cat2, 2 * H, M, H, 2 * H, g->attn.w_out, 2 * H, 1, st, ar.rest(), ar.rest_n()));
        if (g->attn.w_in) TRY(gemm_tn(gtape->dt_text, H, tape0->cat2 + H, 2 * H, M, H, H, g->attn.w_in, H, 1, st, ar.rest(), ar.rest_n()));
        if (g->lstm.w_ih) {
            SF_CHECK_ARG(tape0->emb);
            TRY(gemm_tn(gtape->dgates, 4 * H, tape0->emb, E, M, 4 * H, E, g->lstm.w_ih, E, 1, st, ar.rest(), ar.rest_n()));
        }
        if (g->lstm.w_hh) TRY(gemm_tn(gtape->dgates, 4 * H, h0_all, H, M, 4 * H, H, g->lstm.w_hh, H, 1, st, ar.rest(), ar.rest_n()));
        TRY(colsum_pair(gtape->dgates, 4 * H, M, 4 * H, g->lstm.b_ih, g->lstm.b_hh, ar, st));
    }
    return SF_OK;
}

// ---- TEACHER-FORCED speaker passes (round 5) ------------------------------------------------------------------------
// With teacher forcing the next input word is the target (speaker.py:166-167): the recurrence h_t = LSTM(emb(w_t), h_{t-1})
// does not depend on the attention, the vocabulary projection or the glue of any step.  So the S word steps split into
//   (1) the recurrence alone -- structurally the follower's EncoderLSTM with a given initial state: ONE persistent launch
//       (enc_persist_kernel, 4.5 us per step instead of 11 us for the full persistent word loop and ~50 us per-step), and
//   (2) everything else -- dropout(h1), attention over the path context, h~, vocabulary projection, log-soft-max / NLL /
//       score -- for all S*B rows AT ONCE: five products with M = S*B instead of 5 S launch-bound ones with M = B.
// The backward likewise: the head's backward for all rows at once, then enc_bwd_persist_kernel with the head's dh1 as the
// per-step external gradient.  Same arithmetic per element as the per-step entry points (sf_speaker_words_fwd / _bwd are
// the checkers in tests/test_gpu_speaker_teacher.py).
int sf_speaker_teacher_fwd(const sf_spk_decoder_w* w, int B, int E, int H, int Tp, int vocab, int S, int pad_idx,
                           int eos_idx, const int64_t* targets, float* hs_all, float* cs_all, const float* ctx,
                           const uint8_t* ctx_mask, int64_t* words, uint8_t* ended, float* step_scores, float* nll_term,
                           float* live, const sf_spk_decoder_tape* tape0, const sf_dropout* drop, uint32_t step0, void* ws,
                           size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && targets && hs_all && cs_all && ctx && words && ended && step_scores && nll_term && live && tape0 &&
                 tape0->gates && tape0->cat2 && tape0->t_text && tape0->alpha && tape0->h_tilde && tape0->logit && B > 0 &&
                 S > 0 && Tp > 0 && vocab > 0);
    if (!w->xw_table || (w->flags & SF_SPK_EMB_DROPOUT) || !encoder_persistent_supported(B, H, S)) return SF_ERR_UNSUPPORTED;
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = (hipStream_t)stream;        // (the parameter S shadows the S() cast helper here)
    const size_t BH = (size_t)B * H;
    const int M = S * B, ldv = (vocab + 3) & ~3;
    SF_CHECK_ARG(tape0->h1 == hs_all + BH && tape0->c1 == cs_all + BH);
    float* xchg = ar.take(encoder_persistent_xchg_floats(H));
    int* crow = reinterpret_cast<int*>(ar.take((size_t)M));
    NEED(xchg && crow && ar.tickets());
    // teacher forcing: words[t + 1] = targets[t] (speaker.py:167) -- known before the first step
    if (hipMemcpyAsync(words + B, targets, (size_t)M * sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return SF_ERR_LAUNCH;
    // (1) the recurrence: tokens words[t][b] (time-major: stride B per step), initial state = slot 0 of the tapes
    TRY(encoder_persistent(w->lstm.w_hh, w->lstm.b_ih, w->lstm.b_hh, w->xw_table, words, 1, nullptr, B, H, S,
                           tape0->gates, hs_all, cs_all, nullptr, make_dropout(nullptr, 0), xchg,
                           ar.tickets() + PERSIST_TICKET, st, nullptr, hs_all, cs_all, (long)B));
    if (tape0->emb) TRY(embedding_rows(w->embedding, E, words, M, tape0->emb, st));      // (only the backward's dW_ih reads them)
    // (2) the head over all S*B rows: dropout(h1) with the per-step sites 2 (step0 + t) + 1 (model.py:516) ...
    TRY(dropout_steps(hs_all + BH, H, S, B, H, tape0->cat2 + H, 2 * H, make_dropout(drop, 2 * step0 + 1, 2), 2, st));
    // ... attention over the path context of row m % B, h~ (model.py:517), vocabulary projection (:518)
    TRY(row_mod(crow, M, B, st));
    TRY(softdot_fwd_i(&w->attn, M, Tp, H, nullptr, 0, ctx, ctx_mask, tape0->h_tilde, tape0->alpha, tape0->cat2,
                      tape0->t_text, ar, st, crow));
    TRY(linear_plain(tape0->h_tilde, H, w->w_out, H, w->b_out, M, vocab, H, EPI_NONE, tape0->logit, ldv, ar, st));
    // glue of every step (speaker.py:163-191; teacher feedback: rows are independent, `ended` is an OR)
    return speaker_glue_fwd(M, vocab, ldv, tape0->logit, targets, 0, pad_idx, eos_idx, ended, words + B, step_scores,
                            nll_term, live, st, nullptr, B);
}

int sf_speaker_teacher_bwd(const sf_spk_decoder_w* w, const sf_spk_decoder_g* g, int B, int E, int H, int Tp, int vocab,
                           int S, int pad_idx, const int64_t* words, const int64_t* targets, const float* hs_all,
                           const float* cs_all, const float* ctx, const sf_spk_decoder_tape* tape0, const float* gscale,
                           float* dh_init, float* dc_init, float* dctx, const sf_dropout* drop, uint32_t step0,
                           const sf_spk_decoder_gtape* gtape, float* dcat2, float* ds, float* dh1_ext, void* ws,
                           size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && words && targets && hs_all && cs_all && ctx && tape0 && gscale && dh_init && dc_init && dctx && gtape &&
                 gtape->dlogit && gtape->dpre && gtape->dt_text && gtape->dgates && dcat2 && ds && dh1_ext && B > 0 && S > 0);
    if (!w->xw_table || (w->flags & SF_SPK_EMB_DROPOUT) || (g && g->embedding) || !encoder_persistent_supported(B, H, S) ||
        !ctx_grad_supported(S, Tp, H))
        return SF_ERR_UNSUPPORTED;
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = (hipStream_t)stream;        // (the parameter S shadows the S() cast helper here)
    const size_t BH = (size_t)B * H;
    const int M = S * B, ldv = (vocab + 3) & ~3;
    float* xchg = ar.take(encoder_bwd_persistent_xchg_floats());
    int* crow = reinterpret_cast<int*>(ar.take((size_t)M));
    NEED(xchg && crow && ar.tickets());
    // ---- the head's backward for all S*B rows at once
    TRY(softmax_ce_bwd(M, vocab, ldv, tape0->logit, targets, pad_idx, gscale, gtape->dlogit, st, B));
    TRY(spk_dlogit_to_dht(w, gtape->dlogit, ldv, M, H, vocab, gtape->dpre, ar, st));             // d h~ ...
    TRY(tanh_bwd(tape0->h_tilde, H, gtape->dpre, H, M, H, gtape->dpre, H, st));                  // ... -> d pre, in place
    TRY(row_mod(crow, M, B, st));
    // (dh1_ext receives d dropout(h1) = dcat2[:, H:] + dt W_in; the context gradient is deferred: dcat2 / ds)
    TRY(softdot_bwd_i(&w->attn, nullptr, M, Tp, H, ctx, tape0->alpha, tape0->cat2, tape0->t_text, tape0->h_tilde,
                      gtape->dpre, dh1_ext, H, nullptr, ar, st, gtape->dpre, gtape->dt_text, true, dcat2, ds, crow));
    TRY(ctx_grad_accum(tape0->alpha, ds, dcat2, 2 * H, tape0->t_text, S, B, Tp, H, dctx, st));
    // through dropout(h1): the forward's masks, in place
    TRY(dropout_steps(dh1_ext, H, S, B, H, dh1_ext, H, make_dropout(drop, 2 * step0 + 1, 2), 2, st));
    // ---- the recurrence's backward: all S steps in one persistent launch, dh1_ext[t] the external gradient of h_t
    TRY(encoder_bwd_persistent(w->lstm.w_hh, nullptr, B, H, S, tape0->gates, cs_all, dh1_ext, make_dropout(nullptr, 0),
                               nullptr, nullptr, gtape->dgates, xchg, ar.tickets() + PERSIST_TICKET, st, (long)H,
                               (long)BH, dc_init));
    // d h_init = dgates_0 W_hh
    TRY(data_grad(gtape->dgates, 4 * H, w->lstm.w_hh, w->lstm.w_hh_t, B, 4 * H, H, dh_init, H, 0, ar, st));
    if (g) {
        // every weight gradient as ONE product over the S*B stacked rows (as sf_speaker_words_bwd with a gtape)
        if (g->w_out) TRY(gemm_tn(gtape->dlogit, ldv, tape0->h_tilde, H, M, vocab, H, g->w_out, H, 1, st, ar.rest(), ar.rest_n()));
        if (g->b_out) TRY(colsum(gtape->dlogit, ldv, M, vocab, g->b_out, 1, st, nullptr, ar.rest(), ar.rest_n()));
        if (g->attn.w_out) TRY(gemm_tn(gtape->dpre, H, tape0->cat2, 2 * H, M, H, 2 * H, g->attn.w_out, 2 * H, 1, st, ar.rest(), ar.rest_n()));
        if (g->attn.w_in) TRY(gemm_tn(gtape->dt_text, H, tape0->cat2 + H, 2 * H, M, H, H, g->attn.w_in, H, 1, st, ar.rest(), ar.rest_n()));
        if (g->lstm.w_ih) {
            SF_CHECK_ARG(tape0->emb);
            TRY(gemm_tn(gtape->dgates, 4 * H, tape0->emb, E, M, 4 * H, E, g->lstm.w_ih, E, 1, st, ar.rest(), ar.rest_n()));
        }
        if (g->lstm.w_hh) TRY(gemm_tn(gtape->dgates, 4 * H, hs_all, H, M, 4 * H, H, g->lstm.w_hh, H, 1, st, ar.rest(), ar.rest_n()));
        TRY(colsum_pair(gtape->dgates, 4 * H, M, 4 * H, g->lstm.b_ih, g->lstm.b_hh, ar, st));
    }
    return SF_OK;
}

int sf_speaker_loss_finalize(const float* sum_cnt, const int64_t* words, int eos_idx, int T, int B, float* loss,
                             float* gscale, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(sum_cnt && words && loss && gscale && T > 0 && B > 0);
    return speaker_loss_finalize(sum_cnt, words, eos_idx, T, B, loss, gscale, S(stream));
}

int sf_speaker_glue_bwd(int B, int vocab, int ldv, const float* logit, const int64_t* target,
                        int pad_idx, const float* gscale, float* dlogit, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(logit && target && gscale && dlogit && B > 0 && vocab > 0 && ldv >= vocab);
    return softmax_ce_bwd(B, vocab, ldv, logit, target, pad_idx, gscale, dlogit, S(stream));
}

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
