// What the library knows about a buffer by its ADDRESS (sf_api_util.h: Registry): the fp16 storage tag of a feature
// table, its projected tables, its gate-space rows, and the packed bf16 images of an LSTM's weights -- with everything
// that builds or queries them.  The `*_use` switches and the argument checks stay with their entries.
#include "sf_api_util.h"

namespace sf {

std::atomic<long long> g_proj_steps{0};
std::atomic<long long> g_gate_steps{0};
std::atomic<long long> g_gate_att_steps{0};
std::atomic<long long> g_gate_rec_steps{0};

namespace {

struct Tagged {};                                    // the fp16 tag: being registered is all there is to know
struct WeightPair {
    const float *w_ih, *w_hh;
    bool operator==(const WeightPair& o) const { return w_ih == o.w_ih && w_hh == o.w_hh; }
};
struct PackedPair { const void *ih, *hh; };

// ---- fp16 storage of the feature table (include/sf_hip.h: sf_feature_table_f16) ----------------------------------------
Registry<const void*, Tagged> g_f16_tables;
// ---- projected feature tables (include/sf_hip.h: sf_projected_register) -------------------------------------------------
// One entry per feature table; an entry also names the decoder it belongs to (two of its weights) and the location
// table, and a step whose decoder or location table is another one does not see it.
Registry<const void*, sf_projected> g_proj;
std::atomic<int> g_proj_use{1};             // sf_projected_use
// ---- gate-space rows (include/sf_hip.h: sf_gate_rows_register); an entry names the decoder by its W_ih ---------------------
Registry<const void*, sf_gate_rows> g_gate;
std::atomic<int> g_gate_use{1};             // sf_gate_rows_use
Registry<const void*, sf_gate_rows_attended> g_gate_att;    // sf_gate_rows_attended_register
std::atomic<int> g_gate_att_use{1};         // sf_gate_rows_attended_use
std::atomic<int> g_gate_rec_use{1};         // sf_gate_rows_recurrent_use
// ---- bf16 weight storage of the gate product (include/sf_hip.h: sf_gate_product_bf16_weights) ---------------------------
Registry<WeightPair, PackedPair> g_bf16_pairs;
std::atomic<int> g_bf16w_on{0};

// rows of the feature table one product of the build takes (its output, the largest thing in flight, is 34 MB)
constexpr long long PROJ_CHUNK_ROWS = 16384;
long long g_proj_chunk_rows = PROJ_CHUNK_ROWS;      // sf_debug_projected_chunk_rows

}  // namespace

int table_is_f16(const void* table) { return table && g_f16_tables.find(table, nullptr) ? 1 : 0; }
bool projected_lookup(const void* table, sf_projected* out) {
    return table && g_proj_use.load(std::memory_order_relaxed) && g_proj.find(table, out);
}
bool gate_rows_lookup(const void* table, sf_gate_rows* out) {
    return table && g_gate_use.load(std::memory_order_relaxed) && g_gate.find(table, out);
}
bool gate_rows_attended_lookup(const void* table, sf_gate_rows_attended* out) {
    return table && g_gate_att_use.load(std::memory_order_relaxed) && g_gate_att.find(table, out);
}
bool gate_rows_recurrent_on() { return g_gate_rec_use.load(std::memory_order_relaxed) != 0; }
bool bf16_packed(const float* w_ih, const float* w_hh, const void* (&packed)[2]) {
    if (!g_bf16w_on.load(std::memory_order_relaxed) || sf::g_nt_force_f32) return false;
    PackedPair p;
    if (!g_bf16_pairs.find(WeightPair{w_ih, w_hh}, &p)) return false;
    packed[0] = p.ih;
    packed[1] = p.hh;
    return true;
}

}  // namespace sf

using namespace sf;

extern "C" {

size_t sf_pack_bf16_bytes(int rows, int K) { return sf::pack_bf16_bytes(rows, K); }
int sf_pack_bf16(const float* w, int ld, int rows, int K, void* out, sf_stream stream) {
    SF_ENTER();
    return sf::pack_bf16(w, ld, rows, K, out, S(stream));
}
int sf_lstm_weights_bf16(const float* w_ih, const float* w_hh, const void* packed_ih, const void* packed_hh) {
    SF_CHECK_ARG(w_ih && (packed_ih || !packed_hh) && (!packed_ih || !w_hh == !packed_hh));
    if (!packed_ih) return g_bf16_pairs.forget(WeightPair{w_ih, w_hh});
    return g_bf16_pairs.put(WeightPair{w_ih, w_hh}, PackedPair{packed_ih, packed_hh});
}
void sf_gate_product_bf16_weights(int on) { g_bf16w_on.store(on ? 1 : 0, std::memory_order_relaxed); }
int sf_gate_product_bf16_weights_is_on(void) { return g_bf16w_on.load(std::memory_order_relaxed); }
int sf_gate_product_bf16_supported(int M, int K1, int K2, int N) {
    if (K2 < 0) return 0;
    const int K[2] = {K1, K2};
    return sf::bf16w_supported(M, N, K, K2 ? 2 : 1) ? 1 : 0;
}

int sf_feature_table_f16(const void* table, int on) {
    SF_CHECK_ARG(table);
    return on ? g_f16_tables.put(table, Tagged{}) : g_f16_tables.forget(table);
}
int sf_feature_table_is_f16(const void* table) { return table_is_f16(table); }

int sf_projected_ld(int H) { return H > 0 ? projected_ld(H) : 0; }
int sf_projected_register(const void* table, const sf_projected* p) {
    SF_CHECK_ARG(table);
    if (!p) return g_proj.forget(table);
    SF_CHECK_ARG(p->pv && p->pa && p->lv && p->la && p->loc_table && p->key_v && p->key_a && p->H > 0 && p->H % 4 == 0 &&
                 p->ld == projected_ld(p->H) && p->V > 0 && p->IMG > 0 && p->LOC > 0);
    return g_proj.put(table, *p);
}
int sf_projected_registered(const void* table, sf_projected* out) { return table && g_proj.find(table, out) ? 1 : 0; }
void sf_projected_use(int on) { g_proj_use.store(on ? 1 : 0, std::memory_order_relaxed); }
int sf_projected_is_used(void) { return g_proj_use.load(std::memory_order_relaxed); }
long long sf_projected_steps(void) { return g_proj_steps.load(std::memory_order_relaxed); }
int sf_projected_text_groups_plan(int B, int L, int with_partials, int slots, int product_blocks, int* grid) {
    if (B < 1 || L < 1 || slots < 0 || product_blocks < 0) return 0;
    return sf::proj_text_groups_plan(B, L, with_partials != 0, product_blocks, slots, 0, grid);
}
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
    if (!g) return g_gate.forget(table);
    SF_CHECK_ARG(g->gu && g->gl && g->key_w && g->H > 0 && g->H % 4 == 0 && g->V > 0 && g->IMG > 0 && g->LOC > 0);
    return g_gate.put(table, *g);
}
int sf_gate_rows_registered(const void* table, sf_gate_rows* out) { return table && g_gate.find(table, out) ? 1 : 0; }
void sf_gate_rows_use(int on) { g_gate_use.store(on ? 1 : 0, std::memory_order_relaxed); }
int sf_gate_rows_is_used(void) { return g_gate_use.load(std::memory_order_relaxed); }
long long sf_gate_rows_steps(void) { return g_gate_steps.load(std::memory_order_relaxed); }

int sf_gate_rows_attended_build(const float* w_ih, const float* table, long long n_rows, int IMG, int LOC, int H, float* gf,
                                void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w_ih && table && gf && n_rows > 0 && IMG > 0 && IMG % 4 == 0 && LOC > 0 && LOC % 16 == 0 && H > 0 &&
                 H % 4 == 0);
    if (table_is_f16(table)) return SF_ERR_UNSUPPORTED;
    const int F = IMG + LOC, G = 4 * H;
    Arena ar = arena(ws, ws_bytes);
    hipStream_t st = S(stream);
    // as gu, against the image columns of the ATTENDED half, W_ih[:, F:F+IMG]
    for (long long r0 = 0; r0 < n_rows; r0 += g_proj_chunk_rows) {
        const int m = (int)std::min<long long>(g_proj_chunk_rows, n_rows - r0);
        TRY(linear_plain(table + (size_t)r0 * IMG, IMG, w_ih + F, 2 * F, nullptr, m, G, IMG, EPI_NONE, gf + (size_t)r0 * G, G, ar,
                         st));
    }
    return SF_OK;
}
int sf_gate_rows_attended_register(const void* table, const sf_gate_rows_attended* g) {
    SF_CHECK_ARG(table);
    if (!g) return g_gate_att.forget(table);
    SF_CHECK_ARG(g->gf && g->key_w && g->H > 0 && g->H % 4 == 0 && g->V > 0 && g->IMG > 0 && g->LOC > 0);
    return g_gate_att.put(table, *g);
}
int sf_gate_rows_attended_registered(const void* table, sf_gate_rows_attended* out) {
    return table && g_gate_att.find(table, out) ? 1 : 0;
}
void sf_gate_rows_attended_use(int on) { g_gate_att_use.store(on ? 1 : 0, std::memory_order_relaxed); }
int sf_gate_rows_attended_is_used(void) { return g_gate_att_use.load(std::memory_order_relaxed); }
long long sf_gate_rows_attended_steps(void) { return g_gate_att_steps.load(std::memory_order_relaxed); }
int sf_gate_rows_attended_supported(int H, int LOC) {
    return H > 0 && LOC > 0 && H % 4 == 0 && LOC % 4 == 0 && proj_partials_supported(4 * H, LOC) &&
           short_gate_fused(LOC, H) ? 1 : 0;
}
void sf_gate_rows_recurrent_use(int on) { g_gate_rec_use.store(on ? 1 : 0, std::memory_order_relaxed); }
int sf_gate_rows_recurrent_is_used(void) { return g_gate_rec_use.load(std::memory_order_relaxed); }
long long sf_gate_rows_recurrent_steps(void) { return g_gate_rec_steps.load(std::memory_order_relaxed); }
int sf_gate_rows_recurrent_supported(int B, int H, int LOC) {
    int mt = 0, cpw = 0;
    return B > 0 && sf_gate_rows_attended_supported(H, LOC) && recurrent_row_cell(LOC, H) &&
           plan_detail::small_shape(B, 4 * H, (H + 15) / 16, &mt, &cpw) && pair_proj_score_hh_accepts(SmallInst{mt, cpw}) ? 1 : 0;
}

}  // extern "C"
