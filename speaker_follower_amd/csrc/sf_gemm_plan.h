// The GEMM dispatch as pure host code: which kernel instantiation forms a product, on what grid, with how many K (or
// row) splits and with what workspace layout.  Nothing here launches, allocates or touches a pointer, and no HIP header
// is included: the file compiles with a plain C++17 compiler, which is how tests/test_gemm_plan_host.py asks it for the
// kernel of a shape without a GPU.  sf_gemm.hip issues what these plans say ("GEMM dispatch: plan and issue").
#pragma once
#include <algorithm>
#include <cstddef>

namespace sf {

// ---- the tile constants the decision reads (the kernels of sf_gemm.hip include this file: one definition) -------------
constexpr int SMALL_WAVES = 8;                       // waves = K slices of a short-reduction block (sf_gemm_small.h)
constexpr int TBK = 64, TLD = TBK + 8;               // gemm_nt_tiled_kernel: stage depth, LDS row stride in dwords
constexpr int SPL_ROWB = 128;                        // gemm_nt_split_kernel: bytes per row and plane (64 bf16)
constexpr int BW_STAGE_BYTES = 2 * 64 * 16;          // packed bf16 weights: bytes per n-tile and stage
constexpr int NB_T = 128, NB_K = 32, NB_PLANE = NB_T * 64;   // gemm_nt_big_kernel: tile, stage depth, bytes per plane and stage
constexpr int NB_GROUP = 8;                          // products of one gemm_nt_big_group_kernel launch
constexpr int TR_GROUP = 16;                         // transposes of one transpose_group_kernel launch
constexpr int TNS_B = 128;                           // gemm_tn_split_kernel: block tile
constexpr int TNS_LDS = 2 * 3 * TNS_B * 128;         // ... its stage buffer: 2 operands x 3 planes x 16 KB
constexpr int TNT_B = 128;                           // gemm_tn_tiled_kernel: block tile

// ---- the instantiations that exist -------------------------------------------------------------------------------------
struct SmallInst { int mt, cpw; };
constexpr int SMALL_INSTS = 10;                      // gemm_nt_small_kernel / gemm_nt_small_x_kernel <MT, CPW>
constexpr SmallInst SMALL_INST[SMALL_INSTS] = {{1, 2}, {1, 4}, {1, 8}, {1, 16}, {1, 18}, {2, 2}, {2, 4}, {2, 8}, {4, 2}, {4, 4}};
constexpr int NT_MT_MAX = 8;                         // gemm_nt_kernel, _split, _tiled, _bf16w <MT>: MT = 1 .. 8
constexpr int NN_INSTS = 4;
constexpr int NN_INST[NN_INSTS] = {1, 2, 4, 7};      // gemm_nn_kernel<MT>

// position in the table (past its end when there is no such instantiation)
constexpr int small_inst(int mt, int cpw) {
    int i = 0;
    while (i < SMALL_INSTS && (SMALL_INST[i].mt != mt || SMALL_INST[i].cpw != cpw)) ++i;
    return i;
}
constexpr int nn_inst(int mt) {
    int i = 0;
    while (i < NN_INSTS && NN_INST[i] != mt) ++i;
    return i;
}

// The decoder's step with ALL THREE halves of its gates as rows (lstm_step_rows_kernel<1|2>: action half, attended image
// half, recurrent half + biases): what is left of the product is K_x columns of x, 8 waves of <= 2 chunks of 16 over a
// 32-row x 8-unit patch.  A pure function of the shape, like short_gate_fused (sf_api_util.h), whose step it replaces.
inline bool recurrent_row_cell(int K_x, int H) { return K_x > 0 && K_x <= 256 && K_x % 4 == 0 && H > 0 && H % 8 == 0; }

// Epilogue applied by the split-K reduce pass (or inline when there is a single split).
enum Epi : int {
    EPI_NONE = 0,    // y = acc + bias
    EPI_TANH = 1,    // y = tanh(acc + bias)
    EPI_MUL = 2,     // y = (acc + bias) * mul[n]         (EltwiseProdScoring fold)
    EPI_TANHBWD = 3, // y = (acc + bias) * (1 - aux[m,n]^2)   (backward through h~ = tanh(.))
};

// The debug switches of include/sf_hip.h that steer the dispatch, as one value: sf_gemm.hip snapshots its g_* words into
// this at every call; the plan functions read nothing else.
struct GemmSwitches {
    int force_f32;           // sf_debug_gate_product_f32 / sf_gate_product_strict: no bf16 matrix-core kernels
    int big, big_ksplit;     // sf_debug_many_row_product bit 0: M >= 512 on gemm_nt_big_kernel; bit 1 clear: its raw-slab K splits
    int tn_split_min_rows;   // sf_debug_tn_split_min_rows: gemm_tn_split_kernel from this many rows on
    int tn_group;            // sf_debug_grouped_weight_gradients
};

// = SF_OK, SF_ERR_UNSUPPORTED, SF_ERR_WORKSPACE of include/sf_hip.h (asserted in sf_gemm.hip)
enum PlanStatus : int { PLAN_OK = 0, PLAN_UNSUPPORTED = 2, PLAN_WORKSPACE = 4 };

struct PlanGrid { int x, y, z; };

namespace plan_detail {

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
constexpr size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }

inline int pick_ksplit(int waves_per_split, int chunks) {
    // aim for ~2 waves per SIMD over the chip (1024 SIMDs), at least 4 16-deep chunks per split,
    // and at most 8 partial slabs (each split costs one extra write + read of the output)
    int ks = (2048 + waves_per_split - 1) / waves_per_split;
    ks = std::min(ks, std::max(1, chunks / 4));
    return std::max(1, std::min(ks, 8));
}

// Short-reduction path: K <= 1024 and a small output (decode-step Linears).  Returns false when the
// streaming kernel should be used instead.
inline bool small_shape(int M, int N, int chunks, int* mt, int* cpw) {
    const int mtiles = cdiv(M, 16), ntiles = cdiv(N, 16);
    if (chunks > 144 || (long)mtiles * ntiles > (chunks > 64 ? 512 : 2048)) return false;
    if (chunks > 128 && (long)mtiles * ntiles > 128) return false;   // (K = 2176 -> 256: the dq / dr products)
    const int c = cdiv(chunks, SMALL_WAVES);              // chunks per wave: 1..18
    *cpw = c <= 2 ? 2 : (c <= 4 ? 4 : (c <= 8 ? 8 : (c <= 16 ? 16 : 18)));
    int m = std::max(1, std::min(mtiles, 32 / *cpw - 1)); // <= 32 float4 of loads per lane
    m = m >= 4 ? 4 : (m >= 2 ? 2 : 1);
    // a CU sustains only ~20-35 GB/s of loads, so what matters is the bytes ONE block pulls
    // (16 W rows + 16*m A rows, K deep): prefer more, lighter blocks until the chip is covered
    while (m > 1 && ntiles * cdiv(mtiles, m) < 224) m >>= 1;
    *mt = m;
    return true;
}

inline void nt_shape(int M, int N, int Ktot_chunks, int* mt, int* mblocks, int* ks) {
    const int mtiles = cdiv(M, 16), ntiles = cdiv(N, 16);
    if (Ktot_chunks <= 64) {
        // short reduction with a large output (the hoisted encoder input product): never split K
        int m = 1;
        while (m < 8 && (long)ntiles * cdiv(mtiles, m) > 4096) m *= 2;
        *mt = std::min(m, mtiles);
        *mblocks = cdiv(mtiles, *mt);
        *ks = 1;
        return;
    }
    *mt = mtiles <= 8 ? mtiles : 8;
    *mblocks = cdiv(mtiles, *mt);
    *ks = pick_ksplit(ntiles * *mblocks, Ktot_chunks);
    // the LDS-tiled kernel runs one workgroup per CU: a grid of more than 256 of them (34 n-tiles x 8
    // splits for the [100,2048] x [2048,2176] input gradient) pays a second, nearly empty round
    if (*mblocks == 1 && Ktot_chunks >= 128)
        while (*ks > 1 && cdiv(N, 64) * *ks > 256) --*ks;
}

// dynamic LDS of gemm_nt_split_kernel<MT> and gemm_nt_bf16w_kernel<MT>: the stage planes, or the K halves' meeting place
inline size_t split_lds(int mt) {
    return std::max<size_t>((size_t)2 * 3 * (((mt + 1) / 2) * 32) * SPL_ROWB, (size_t)4 * mt * 64 * 16);
}

// K splits of a many-row product over M reduction rows whose launch holds `tiles` 128 x 128 tiles in all: up to `budget`
// workgroups (gemm_tn: 256, one round of the chip; gemm_tn_group: 768, ~3 rounds between its products)
inline int many_row_ksplit(int M, int tiles, int budget) {
    return std::max(1, std::min(std::min(16, budget / std::max(1, tiles)), cdiv(M, NB_K) / 4));
}

}  // namespace plan_detail

// ---- NT: y[M,N] = epi(sum_s A_s W_s^T + bias), linear_nt ---------------------------------------------------------------
inline bool bf16w_supported(int M, int N, const int* K, int nseg) {
    bool ok = M >= 1 && M <= 128 && N >= 1 && nseg >= 1 && nseg <= 3;
    for (int s = 0; ok && s < nseg; ++s) ok = K[s] > 0 && K[s] % TBK == 0;
    return ok;
}

enum NtFamily : int { NT_SMALL, NT_BF16W, NT_BIG, NT_SPLIT, NT_TILED, NT_STREAM };

struct NtAsk {
    int M, N, K[3], nseg;    // K: the segment depths
    bool raw_slabs, ksplit_out, packed_w;   // the caller sums the K-split slabs itself; can be told their number; gives bf16 weights
    int epi;                 // Epi
    bool accumulate;
    bool addend, r1_s;       // the short-reduction kernel's extras (with EPI_TANHBWD)
    size_t ws_floats;        // workspace on offer (0: none)
};
struct NtPlan {
    int status;              // PlanStatus; nothing else is meaningful unless PLAN_OK
    NtFamily family;
    int mt, cpw;             // template arguments (cpw: NT_SMALL only)
    bool extras;             // NT_SMALL: gemm_nt_small_x_kernel
    PlanGrid grid;
    int block, ksplit;
    size_t lds, ws_floats;   // dynamic LDS bytes; workspace it uses
    bool slabs;              // the product is written as [ksplit][M][N] slabs at the workspace's start, bias and epilogue left out
    bool reduce;             // a reduce_slabs_kernel launch follows (bias, epilogue, accumulate)
};

inline NtPlan plan_nt(const NtAsk& q, const GemmSwitches& sw) {
    using namespace plan_detail;
    const int M = q.M, N = q.N;
    NtPlan p{};
    p.status = PLAN_OK;
    p.ksplit = 1;
    int chunks = 0, mt, mblocks, ks;
    for (int s = 0; s < q.nseg; ++s) chunks += cdiv(q.K[s], 16);
    // 1. bf16-stored weights: raw slabs only, the K splits of nt_shape (what the caller's workspace was sized for), all
    //    rows in one block
    if (q.packed_w && q.raw_slabs && !sw.force_f32 && bf16w_supported(M, N, q.K, q.nseg)) {
        nt_shape(M, N, chunks, &mt, &mblocks, &ks);
        p.family = NT_BF16W;
        p.mt = cdiv(M, 16);
        p.ws_floats = (size_t)ks * M * N;
        if (q.ws_floats < p.ws_floats) p.status = PLAN_WORKSPACE;
        p.grid = {cdiv(N, 64), ks, 1};
        p.block = 512;
        p.lds = split_lds(p.mt);
        p.ksplit = ks;
        p.slabs = true;
        return p;
    }
    // 2. the short-reduction kernel
    if (!q.raw_slabs && q.nseg <= 2 && small_shape(M, N, chunks, &p.mt, &p.cpw)) {
        p.family = NT_SMALL;
        p.extras = q.addend || q.r1_s || q.epi == EPI_TANHBWD;
        p.grid = {cdiv(N, 16), cdiv(cdiv(M, 16), p.mt), 1};
        p.block = SMALL_WAVES * 64;
        return p;
    }
    // 3. many rows: 128 x 128 tiles through LDS on the bf16 matrix cores (gemm_nt_big_kernel)
    // (raw_slabs: the caller sums split-K slabs itself -- the LSTM cell kernel; here ONE slab without bias)
    bool big = M >= 512 && N >= 64 && chunks >= 4 && !q.r1_s && sw.big && (q.epi == EPI_NONE || q.epi == EPI_TANH) &&
               !(q.accumulate && q.epi != EPI_NONE) && (!q.raw_slabs || q.ws_floats >= (size_t)M * N);
    for (int s = 0; s < q.nseg; ++s) big = big && q.K[s] >= NB_K;         // (a partial last stage per segment is fine)
    if (big) {
        const int tiles = cdiv(M, NB_T) * cdiv(N, NB_T);
        int kb = 1;
        // The consumer adds the slabs up anyway, so K splits are free of a reduce launch: take them when the tile
        // count wastes a round of the 256 CUs (the beam step's 2 560 x 2 048: 320 tiles = 2 rounds; 3 splits =
        // 960 units = 4 rounds of a third each).  Cost of a split: one more slab written and read (M N floats).
        if (q.raw_slabs && q.ksplit_out && sw.big_ksplit) {
            int stages = 0;
            for (int s = 0; s < q.nseg; ++s) stages += cdiv(q.K[s], NB_K);
            double best = (double)cdiv(tiles, 256);
            for (int c = 2; c <= 3; ++c) {
                if (q.ws_floats < (size_t)c * M * N || stages < 16 * c) break;
                const double t = (double)cdiv(tiles * c, 256) / c + 0.04 * (c - 1);
                if (t < best - 1e-9) { best = t; kb = c; }
            }
        }
        p.family = NT_BIG;
        p.grid = {tiles, kb, 1};
        p.block = 512;
        p.lds = (size_t)2 * 6 * NB_PLANE;
        p.ksplit = kb;
        p.slabs = q.raw_slabs;
        p.ws_floats = q.raw_slabs ? (size_t)kb * M * N : 0;
        return p;
    }
    // 4. the extras exist in the short-reduction kernel only
    if (q.addend || q.r1_s || q.epi == EPI_TANHBWD) {
        p.status = PLAN_UNSUPPORTED;
        return p;
    }
    // 5. one block of rows with a deep reduction through LDS (bf16x6 split or fp32), else the streaming kernel
    nt_shape(M, N, chunks, &mt, &mblocks, &ks);
    p.mt = mt;
    p.ksplit = ks;
    p.slabs = ks > 1 || q.raw_slabs;           // (raw slabs with ks == 1: slab 0 is written without bias)
    p.reduce = ks > 1 && !q.raw_slabs;
    p.ws_floats = p.slabs ? (size_t)ks * M * N : 0;
    if (q.ws_floats < p.ws_floats) {
        p.status = PLAN_WORKSPACE;
        return p;
    }
    bool tiled = mblocks == 1 && chunks >= 128 && N % 64 == 0 && (p.slabs || q.epi == EPI_NONE);
    for (int s = 0; s < q.nseg; ++s) tiled = tiled && q.K[s] % TBK == 0;
    if (tiled) {
        // fp32 accuracy on the bf16 matrix cores (gemm_nt_split_kernel): 6/16 of the fp32-MFMA time
        const bool split = M <= 128 && !sw.force_f32;
        p.family = split ? NT_SPLIT : NT_TILED;
        p.grid = {N / 64, ks, 1};
        p.block = 512;
        p.lds = split ? split_lds(mt) : (size_t)2 * (mt * 16 + 64) * TLD * sizeof(float);
    } else {
        p.family = NT_STREAM;
        p.grid = {cdiv(N, 64), ks, mblocks};
        p.block = 256;
    }
    return p;
}

// ---- NN: y[M,N] (+)= A[M,K] W[K,N], gemm_nn_ws -------------------------------------------------------------------------
struct NnPlan {
    int mt, mblocks, ks;
    PlanGrid grid;
    size_t ws_floats;        // ks > 1: [ks][M][N] slabs, then reduce_slabs_kernel
};
inline NnPlan plan_nn(int M, int N, int K, size_t ws_floats) {
    using namespace plan_detail;
    const int mtiles = cdiv(M, 16);
    NnPlan p{};
    p.mt = mtiles <= 1 ? 1 : (mtiles <= 2 ? 2 : (mtiles <= 4 ? 4 : 7));
    p.mblocks = cdiv(mtiles, p.mt);
    p.ks = pick_ksplit(cdiv(N, 64) * p.mblocks, cdiv(K, 16));
    if (p.ks > 1 && ws_floats < (size_t)p.ks * M * N) p.ks = 1;       // degrade, still correct
    p.grid = {cdiv(N, 256), p.ks, p.mblocks};
    p.ws_floats = p.ks > 1 ? (size_t)p.ks * M * N : 0;
    return p;
}

// workspace (in floats) with which gemm_nn_ws splits as it likes
inline size_t gemm_nn_ws_floats(int M, int N, int K) { return plan_nn(M, N, K, ~(size_t)0).ws_floats; }

// ---- TN: out[P,Q] (+)= Y[M,P]^T X[M,Q], gemm_tn ------------------------------------------------------------------------
// The leading columns of a LARGE gemm_tn output [P,Q] that fill whole rounds of the chip's 1024 SIMDs with 64 x 64 wave
// tiles (dW_ih of the decoder LSTM: 2176 tiles = 2.125 per SIMD, so some SIMDs would run 3); the narrow remainder is a
// product of its own (a row split or the many-row kernel spreads it over the chip).  Q when the output is not cut.
inline int gemm_tn_main_columns(int M, int P, int Q) {
    using namespace plan_detail;
    const int waves = cdiv(Q, 64) * cdiv(P, 64);
    const int pb = cdiv(P, 64), qb = cdiv(Q, 256);
    const int rem = waves % 1024;
    if (!(waves > 1024 && rem > 0 && rem <= 384 && rem % (4 * pb) == 0)) return Q;
    const int r = rem / (4 * pb);                       // column blocks of 256 in the remainder
    const int q_main = (qb - r) * 256, q_tail = Q - q_main;
    if (!(r < qb && q_tail > 0)) return Q;
    const int tail_waves = cdiv(q_tail, 64) * pb;
    const int tail_ms = std::min(16, std::max(1, 1024 / tail_waves));
    if (!(tail_ms > 1 && M / 64 >= tail_ms)) return Q;
    return q_main;
}

// Whether gemm_tn runs this product as an NT product of the transposed operands on the many-row kernel
inline bool tn_as_many_row(int M, int P, int Q, const GemmSwitches& sw) {
    return sw.big && !sw.force_f32 && M >= 1024 && M % 4 == 0 && P >= 64 && Q >= 64 &&
           (size_t)P * Q <= (size_t)1536 * 1024 && !(P % TNS_B == 0 && Q % TNS_B == 0 && M >= sw.tn_split_min_rows);
}

enum TnFamily : int { TN_MANY_ROW, TN_SPLIT, TN_TILED, TN_STREAM, TN_COLUMN_CUT };

struct TnPart {              // one product on one kernel
    TnFamily family;
    int splits;              // TN_MANY_ROW: K splits of gemm_nt_big_kernel; else row splits (msplit); > 1: slabs + reduce_slabs_kernel
    PlanGrid grid;
    size_t off_xt;           // TN_MANY_ROW: Y^T [P,M] at the workspace's start, X^T [Q,M] here
    size_t off_slabs;        // [splits][P][Q] slabs (0 unless TN_MANY_ROW)
    size_t ws_floats;
};
struct TnPlan : TnPart {
    int q_main;              // TN_COLUMN_CUT: columns [0, q_main) are `main`, the rest `tail`, each a product of its own
    TnPart main, tail;       // that runs one after the other from the workspace's start
};

namespace plan_detail {

inline TnPart plan_tn_part(int M, int P, int Q, int ldy, size_t ws_floats, const GemmSwitches& sw) {
    TnPart p{};
    auto row_split = [&](int ms) {          // every row split degrades to none on a short workspace
        if (ms > 1 && ws_floats < (size_t)ms * P * Q) ms = 1;
        p.splits = ms;
        p.ws_floats = ms > 1 ? (size_t)ms * P * Q : 0;
        return ms;
    };
    // 1. a SMALL weight matrix with a deep reduction as an NT product of the two TRANSPOSED operands on the many-row kernel
    if (tn_as_many_row(M, P, Q, sw)) {
        const int tiles = cdiv(P, NB_T) * cdiv(Q, NB_T), ks = many_row_ksplit(M, tiles, 256);
        const size_t off_x = round64((size_t)P * M), off_s = off_x + round64((size_t)Q * M);
        const size_t need = off_s + (ks > 1 ? (size_t)ks * P * Q : 0);
        if (ws_floats >= need) {
            p.family = TN_MANY_ROW;
            p.splits = ks;
            p.grid = {tiles, ks, 1};
            p.off_xt = off_x;
            p.off_slabs = off_s;
            p.ws_floats = need;
            return p;
        }
    }
    // 2. bf16x6 split products (gemm_tn_split_kernel) where they are faster: deep reductions (see the kernel's note)
    if (P % TNS_B == 0 && Q % TNS_B == 0 && M >= sw.tn_split_min_rows && !sw.force_f32) {
        const int blocks = (P / TNS_B) * (Q / TNS_B);
        const int ms = row_split(blocks >= 512 ? 1 : std::min(16, std::max(1, std::min(512 / blocks, M / 256))));
        p.family = TN_SPLIT;
        p.grid = {Q / TNS_B, P / TNS_B, ms};
        return p;
    }
    // 3. LDS-tiled kernel: 128 x 128 per block; small outputs split the batch rows into slabs
    if (P >= 128 && Q >= 128 && ldy >= 128 && M >= 4096) {   // (measured: pays for the deep encoder reductions)
        const int blocks = cdiv(Q, TNT_B) * cdiv(P, TNT_B);
        const int ms = row_split(std::min(std::min(16, std::max(1, 768 / blocks)), std::max(1, M / 64)));
        p.family = TN_TILED;
        p.grid = {cdiv(Q, TNT_B), cdiv(P, TNT_B), ms};
        return p;
    }
    // 4. Wave quantisation: a large output whose 64 x 64 wave tiles are a little more than a whole number of rounds over
    //    the chip's 1024 SIMDs is cut into the columns that fill whole rounds and a narrow remainder, which a row split
    //    spreads over the chip on its own -- only if the tail's slabs fit
    const int waves = cdiv(Q, 64) * cdiv(P, 64);
    const int q_tail = Q - gemm_tn_main_columns(M, P, Q);
    if (q_tail > 0) {
        const int tail_ms = std::min(16, std::max(1, 1024 / (cdiv(q_tail, 64) * cdiv(P, 64))));
        if (ws_floats >= (size_t)tail_ms * P * q_tail) {
            p.family = TN_COLUMN_CUT;
            return p;
        }
    }
    // 5. A small weight matrix with a deep reduction (e.g. [256, 2176] over 2000 stacked rows) is a handful of waves each
    //    walking all M rows: split the rows over grid.z into slabs and add them up (deterministic order) until the chip
    //    is covered.
    const int ms = row_split(std::min(std::min(16, std::max(1, 1024 / waves)), std::max(1, M / 64)));
    p.family = TN_STREAM;
    p.grid = {cdiv(Q, 256), cdiv(P, 64), ms};
    return p;
}

}  // namespace plan_detail

inline TnPlan plan_tn(int M, int P, int Q, int ldy, size_t ws_floats, const GemmSwitches& sw) {
    TnPlan p{};
    static_cast<TnPart&>(p) = plan_detail::plan_tn_part(M, P, Q, ldy, ws_floats, sw);
    if (p.family == TN_COLUMN_CUT) {
        // Neither half is cut again: the main columns hold a whole number of rounds (remainder 0), the tail fewer than
        // one round, and gemm_tn_main_columns cuts only above one round with a remainder.
        p.q_main = gemm_tn_main_columns(M, P, Q);
        p.main = plan_detail::plan_tn_part(M, P, p.q_main, ldy, ws_floats, sw);
        p.tail = plan_detail::plan_tn_part(M, P, Q - p.q_main, ldy, ws_floats, sw);
        p.ws_floats = std::max(p.main.ws_floats, p.tail.ws_floats);
    }
    return p;
}

// ---- several weight gradients in three launches, gemm_tn_group ---------------------------------------------------------
// A job is any struct with the members M, P, Q, ldy, ldx and Y, X of sf_gemm.h's TnJob.  Y and X only say WHICH operands
// these are: they are compared, never followed (an operand two products share is transposed once).
struct TnGroupPlan {
    bool grouped;            // false: every job goes through gemm_tn, one by one (nothing below is meaningful)
    int n, job[NB_GROUP];    // the grouped jobs by their positions in the caller's list; the others go through gemm_tn
    int ks[NB_GROUP], yt[NB_GROUP], xt[NB_GROUP];     // their K splits, and which transposes are their operands
    size_t off_slabs[NB_GROUP];          // ks > 1: [ks][P][Q] slabs
    int ntr;                 // the distinct transposes
    struct Tr { int job; bool x; size_t off; } tr[TR_GROUP];     // of operand Y or X of job[.], to this workspace offset
    bool reduce;             // some job has K splits: a reduce_slabs_group_kernel launch follows
    size_t most, ws_floats;  // largest P Q among the split jobs (the reduce grid); workspace it uses
};

template <class Job>
TnGroupPlan plan_tn_group(const Job* jobs, int n, size_t ws_floats, const GemmSwitches& sw) {
    using namespace plan_detail;
    TnGroupPlan g{};
    if (!sw.tn_group || !ws_floats) return g;
    for (int i = 0; i < n && g.n < NB_GROUP; ++i)
        if (tn_as_many_row(jobs[i].M, jobs[i].P, jobs[i].Q, sw)) g.job[g.n++] = i;
    if (g.n < 2) return g;
    // distinct transposes, K splits (every job alike: ~3 rounds of the chip between them), workspace layout
    size_t off = 0;
    auto transposed = [&](int k, bool x) {
        const Job& t = jobs[g.job[k]];
        const auto src = x ? t.X : t.Y;
        const int ld = x ? t.ldx : t.ldy, C = x ? t.Q : t.P;
        for (int j = 0; j < g.ntr; ++j) {
            const Job& u = jobs[g.job[g.tr[j].job]];
            if ((g.tr[j].x ? u.X : u.Y) == src && (g.tr[j].x ? u.ldx : u.ldy) == ld && u.M == t.M &&
                (g.tr[j].x ? u.Q : u.P) == C)
                return j;
        }
        if (g.ntr == TR_GROUP) return -1;
        g.tr[g.ntr] = {k, x, off};
        off += round64((size_t)C * t.M);
        return g.ntr++;
    };
    int tiles_all = 0;
    for (int k = 0; k < g.n; ++k) tiles_all += cdiv(jobs[g.job[k]].P, NB_T) * cdiv(jobs[g.job[k]].Q, NB_T);
    for (int k = 0; k < g.n; ++k) {
        g.yt[k] = transposed(k, false);
        g.xt[k] = g.yt[k] < 0 ? -1 : transposed(k, true);
        if (g.xt[k] < 0) return g;
        g.ks[k] = many_row_ksplit(jobs[g.job[k]].M, tiles_all, 768);
    }
    g.most = 1;
    for (int k = 0; k < g.n; ++k) {
        if (g.ks[k] <= 1) continue;
        const Job& t = jobs[g.job[k]];
        g.off_slabs[k] = off;
        off += round64((size_t)g.ks[k] * t.P * t.Q);
        g.most = std::max(g.most, (size_t)t.P * t.Q);
        g.reduce = true;
    }
    g.ws_floats = off;
    g.grouped = off <= ws_floats;
    return g;
}

// ---- bias gradients: out[N] (+)= sum_m Y[m, n], colsum -----------------------------------------------------------------
struct ColsumPlan {
    int ms;                  // row splits; > 1: partial sums in the workspace, then colsum_finish_kernel
    PlanGrid grid, finish;
    size_t ws_floats;
};

inline ColsumPlan plan_colsum(int M, int N, size_t ws_floats) {
    using namespace plan_detail;
    const int nb = cdiv(N, 64);
    ColsumPlan p{};
    p.ms = std::min(std::min(32, std::max(1, 256 / nb)), std::max(1, M / 64));
    if (p.ms > 1 && ws_floats < (size_t)p.ms * N) p.ms = 1;
    p.grid = {nb, p.ms, 1};
    p.finish = {cdiv(N, 256), 1, 1};
    p.ws_floats = p.ms > 1 ? (size_t)p.ms * N : 0;
    return p;
}

}  // namespace sf
