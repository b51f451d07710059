// fp32 GEMMs on the gfx950 matrix cores (v_mfma_f32_16x16x4_f32: exact f32 FMA chain).
//
// Every Linear / LSTMCell product on the speaker/follower path has a skinny batch dimension
// (M = 100 samples, or M = batch*time for the hoisted encoder input product), so the kernels
// stream the weight operand once, straight from HBM into registers (no LDS round trip: a
// weight tile is used by exactly one wave), keep a column of 16x16 accumulator tiles per wave
// and get their parallelism from N-tiles x K-splits.  The small activation operand is re-read
// by every wave and is served by L1/L2.
//
// Fragment trick: mfma_f32_16x16x4 wants A[i][k] from lane (i = lane&15, k = lane>>4) and
// B[k][j] from lane (j = lane&15, k = lane>>4).  A sum over k is order-independent, so a lane
// loads a float4 of four CONSECUTIVE k (k0 + 4*(lane>>4) + c, c = 0..3) for its row and feeds
// component c to MFMA c: A and B use the same permutation of k, loads are 16 B wide and each
// 16-lane group reads 64 contiguous bytes per row.  For operands whose contiguous dimension is
// the row/column index instead (W[K,N] in dX = dY*W, both operands of dW = dY^T*X) the float4
// runs along that index and defines four "virtual" 16-wide tiles with stride-4 columns, which
// the epilogue writes back as float4.
#include "sf_gemm.h"
#include "sf_gemm_small.h"
#include "sf_kernels.h"
#include "sf_lstm.h"
#include "sf_split.h"

#include <cstdlib>
#include <utility>

namespace sf {

int g_tn_split_min_rows = 4096;   // sf_debug_tn_split_min_rows (tests run the split weight-gradient kernel on small shapes)
int g_nt_big_ksplit = 1;     // sf_debug_many_row_product(on | 2 * no K splits of the raw-slab many-row products)
int g_nt_big = 1;            // sf_debug_many_row_product: M >= 512 products on gemm_nt_big_kernel (0: gemm_nt_kernel, rounds 1-4)
int g_nt_force_f32 = 0;      // sf_debug_gate_product_f32: run the LSTM gate product on v_mfma_f32_16x16x4_f32 (round 1-3 kernel)
int g_tn_group = 1;          // sf_debug_grouped_weight_gradients (0: one gemm_tn per product, the round-5 first form)

namespace {

// ------------------------------------------------------------------------------------------------
// NT: C[M,N] = sum_s A_s[M,K_s] * W_s[N,K_s]^T        (forward Linear; both operands K-contiguous)
// grid (ceil(N/64), ksplit, mblocks), block 256 = 4 waves, wave = MT m-tiles x one 16-col n-tile.
// The k loop runs a 3-deep register prefetch ring: a weight chunk comes straight from HBM
// (~900 cycles) while one chunk's MFMAs take MT*4*32 cycles, so two chunks stay in flight.
// ------------------------------------------------------------------------------------------------
struct NtArgs {
    Seg seg[3];
    int nseg;
    int M, N;
    int chunks_total;      // sum over segments of ceil(K_s / 16)
    int ksplit;
    float* out;            // slab base ([ksplit][M][N], ld = N) or final y when ksplit == 1
    int ldo;               // N for slabs, ldy for direct
    const float* bias;     // direct mode only
    const float* bias2;
    int epi;               // direct mode only: EPI_*
    const float* mul;
    float* y_pre;
    int ldy_pre;
    int accumulate;        // direct mode only
};

template <int MT>
struct Frag {
    float4 b;
    float4 a[MT];
};

template <int MT>
__device__ __forceinline__ void nt_load(Frag<MT>& f, const float* pb, const float* const (&pa)[MT],
                                        int chunk) {
    f.b = ld4(pb + chunk * 16);
#pragma unroll
    for (int t = 0; t < MT; ++t) f.a[t] = ld4(pa[t] + chunk * 16);
}

template <int MT>
__device__ __forceinline__ void nt_mma(const Frag<MT>& f, f32x4 (&acc)[MT]) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = mfma16(comp(f.a[t], c), comp(f.b, c), acc[t]);
}

// Chunks [lo, hi) of one segment.  The steady-state loop body is branch-free (prefetch indices are
// clamped instead of predicated) so that the compiler can keep two chunks of loads in flight behind
// counted s_waitcnt vmcnt(N); a conditional load would force vmcnt(0) at every join.
template <int MT>
__device__ __forceinline__ void nt_segment(const Seg& sg, int lo, int hi, int n,
                                           const int (&mrow)[MT], int kk, f32x4 (&acc)[MT]) {
    const int full = sg.K >> 4;
    const float* pb = sg.W + (size_t)n * sg.ldw + 4 * kk;
    const float* pa[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) pa[t] = sg.A + (size_t)mrow[t] * sg.lda + 4 * kk;
    const int end = min(hi, full);          // full chunks are [lo, end)
    if (lo < end) {
        const int last = end - 1;
        Frag<MT> f0, f1, f2;
        nt_load<MT>(f0, pb, pa, lo);
        nt_load<MT>(f1, pb, pa, min(lo + 1, last));
        int i = lo;
        for (; i + 3 <= end; i += 3) {
            nt_load<MT>(f2, pb, pa, min(i + 2, last));
            nt_mma<MT>(f0, acc);
            nt_load<MT>(f0, pb, pa, min(i + 3, last));
            nt_mma<MT>(f1, acc);
            nt_load<MT>(f1, pb, pa, min(i + 4, last));
            nt_mma<MT>(f2, acc);
        }
        if (i < end) nt_mma<MT>(f0, acc);
        if (i + 1 < end) nt_mma<MT>(f1, acc);
    }
    if (hi > full) {   // K_s % 16 != 0: one partial chunk, float4 granularity (K_s % 4 == 0)
        const bool ok = full * 16 + 4 * kk < sg.K;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        Frag<MT> f;
        f.b = ok ? ld4(pb + full * 16) : z;
#pragma unroll
        for (int t = 0; t < MT; ++t) f.a[t] = ok ? ld4(pa[t] + full * 16) : z;
        nt_mma<MT>(f, acc);
    }
}

template <int MT>
__device__ __forceinline__ void nt_mainloop(const NtArgs& a, int c0, int c1, int n,
                                            const int (&mrow)[MT], int kk, f32x4 (&acc)[MT]) {
    int cs = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (s >= a.nseg) break;
        const Seg sg = a.seg[s];
        const int nch = (sg.K + 15) >> 4;
        const int lo = max(c0, cs) - cs, hi = min(c1, cs + nch) - cs;
        cs += nch;
        if (lo < hi) nt_segment<MT>(sg, lo, hi, n, mrow, kk, acc);
    }
}

template <int MT>
__global__ __launch_bounds__(256) void gemm_nt_kernel(NtArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * 16;
    if (n0 >= a.N) return;
    const int split = blockIdx.y;
    const int m0 = blockIdx.z * (16 * MT);
    const int li = lane & 15, kk = lane >> 4;

    const int n = min(n0 + li, a.N - 1);
    int mrow[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) mrow[t] = min(m0 + 16 * t + li, a.M - 1);

    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int c0 = (int)(((long)split * a.chunks_total) / a.ksplit);
    const int c1 = (int)(((long)(split + 1) * a.chunks_total) / a.ksplit);
    nt_mainloop<MT>(a, c0, c1, n, mrow, kk, acc);

    // D layout: col = lane & 15, row = (lane >> 4) * 4 + r
    const int col = n0 + li;
    if (col >= a.N) return;
    float* out = a.out + (a.ksplit > 1 ? (size_t)split * a.M * a.N : 0);
    float bsum = 0.f;
    if (a.bias) bsum += a.bias[col];
    if (a.bias2) bsum += a.bias2[col];
    const float mulv = a.epi == EPI_MUL ? a.mul[col] : 1.f;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + 16 * t + kk * 4 + r;
            if (row >= a.M) continue;
            float v = acc[t][r] + bsum;
            if (a.epi == EPI_TANH) v = tanhf(v);
            if (a.epi == EPI_MUL) {
                if (a.y_pre) a.y_pre[(size_t)row * a.ldy_pre + col] = v;
                v *= mulv;
            }
            float* o = out + (size_t)row * a.ldo + col;
            *o = (a.accumulate && a.ksplit == 1) ? *o + v : v;
        }
}

// ------------------------------------------------------------------------------------------------
// LDS-tiled NT GEMM for the one MFMA-bound product of the path: the decoder LSTM gates
// [B<=128, 4864] x [2048, 4864]^T.  The register-streaming kernel above feeds the matrix cores with
// "fragment shaped" loads (16 rows x 64 B per wave instruction), which keeps the texture addresser
// busy twice as long as full lines would; here a block stages BK = 64 deep tiles of A (MT*16 rows)
// and W (64 rows) into LDS with full 256-B row segments (16 lanes per row), double buffered through
// registers (next stage's global loads are in flight while the current stage's 16*MT MFMAs per wave
// run), and the four waves read their fragments with conflict-free ds_read_b128 (row stride
// 68 dwords: 16 rows x 4 banks tile the 64 banks exactly).
// grid (N/64, ksplit), block 256; a block's stages lie inside one K segment each (K_s % 64 == 0).
// ------------------------------------------------------------------------------------------------
// Row stride 72 dwords: conflict-free for the ds_read_b128 lane groups of gfx950 ({0-3,12-15,20-27},
// ...: MI355X_MICROARCH.md, LDS table).  68 gave a 2-way conflict in every group
// (SQ_LDS_BANK_CONFLICT = 35 % of SQ_LDS_IDX_ACTIVE).
// (TBK = 64, TLD = TBK + 8: sf_gemm_plan.h)

// 8 waves per block: waves 0-3 take the first half of every 64-deep stage, waves 4-7 the second
// half (two waves per SIMD hide each other's barrier and LDS latencies); the halves meet in LDS.
template <int MT>
__global__ __launch_bounds__(512) void gemm_nt_tiled_kernel(NtArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int AROWS = MT * 16, WROWS = 64;
    constexpr int BUF = (AROWS + WROWS) * TLD;           // floats per stage buffer
    constexpr int APASS = (MT + 1) / 2;                  // 32 rows x 16 float4 per staging pass
    const int tid = threadIdx.x, lane = tid & 63, wave8 = tid >> 6;
    const int wave = wave8 & 3, khalf = wave8 >> 2;
    const int li = lane & 15, kk = lane >> 4;
    // XCD-aware tile map: consecutive workgroup ids go round-robin to the 8 XCDs (each with its own
    // L2).  Give every XCD a contiguous range of (split, n-tile) pairs, so that its L2 only ever
    // holds ITS k-slices of the activation operand (M x K/8) instead of all of A.
    int n0, split;
    {
        const int total = gridDim.x * gridDim.y;
        const int b = blockIdx.x + gridDim.x * blockIdx.y;
        int g = b;
        if ((total & 7) == 0) g = (b & 7) * (total >> 3) + (b >> 3);
        split = g / (int)gridDim.x;
        n0 = (g % (int)gridDim.x) * 64;
    }
    const int ldrow = tid >> 4, ldc4 = tid & 15;         // staging: 32 rows x 16 float4 per pass

    // stage range of this split (stages of 64 k over the concatenated segments)
    const int st0n = a.seg[0].K / TBK;
    const int st1n = a.nseg > 1 ? a.seg[1].K / TBK : 0;
    const int st2n = a.nseg > 2 ? a.seg[2].K / TBK : 0;
    const int stages = st0n + st1n + st2n;
    const int s_lo = (int)(((long)split * stages) / a.ksplit);
    const int s_hi = (int)(((long)(split + 1) * stages) / a.ksplit);

    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    struct Regs {
        float4 a[APASS];
        float4 w[2];
    };
    auto gload = [&](Regs& r, int s) {
        const float* A;
        const float* W;
        int lda, ldw, k0;
        if (s < st0n) {
            A = a.seg[0].A; W = a.seg[0].W; lda = a.seg[0].lda; ldw = a.seg[0].ldw; k0 = s * TBK;
        } else if (s < st0n + st1n) {
            A = a.seg[1].A; W = a.seg[1].W; lda = a.seg[1].lda; ldw = a.seg[1].ldw; k0 = (s - st0n) * TBK;
        } else {
            A = a.seg[2].A; W = a.seg[2].W; lda = a.seg[2].lda; ldw = a.seg[2].ldw;
            k0 = (s - st0n - st1n) * TBK;
        }
#pragma unroll
        for (int p = 0; p < APASS; ++p) {
            const int row = min(p * 32 + ldrow, a.M - 1);
            r.a[p] = ld4(A + (size_t)row * lda + k0 + 4 * ldc4);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int row = min(n0 + p * 32 + ldrow, a.N - 1);
            r.w[p] = ld4(W + (size_t)row * ldw + k0 + 4 * ldc4);
        }
    };
    auto lstore = [&](const Regs& r, int buf) {
        float* As = smem + buf * BUF;
        float* Ws = As + AROWS * TLD;
#pragma unroll
        for (int p = 0; p < APASS; ++p)
            if (p * 32 + ldrow < AROWS)
                *reinterpret_cast<float4*>(As + (p * 32 + ldrow) * TLD + 4 * ldc4) = r.a[p];
#pragma unroll
        for (int p = 0; p < 2; ++p)
            *reinterpret_cast<float4*>(Ws + (p * 32 + ldrow) * TLD + 4 * ldc4) = r.w[p];
    };
    // one global load of the staging set (piece 0..APASS+1), issued between groups of 7 MFMAs: six
    // back-to-back loads from all 8 waves right after the barrier stall every wave on the address
    // path with the matrix pipe idle (timestamped: ~0.4 us per stage)
    struct StageSrc {
        const float* A;
        const float* W;
        int lda, ldw;
    };
    auto stage_src = [&](int s) {
        const float* A;
        const float* W;
        int lda, ldw, k0;
        if (s < st0n) {
            A = a.seg[0].A; W = a.seg[0].W; lda = a.seg[0].lda; ldw = a.seg[0].ldw; k0 = s * TBK;
        } else if (s < st0n + st1n) {
            A = a.seg[1].A; W = a.seg[1].W; lda = a.seg[1].lda; ldw = a.seg[1].ldw; k0 = (s - st0n) * TBK;
        } else {
            A = a.seg[2].A; W = a.seg[2].W; lda = a.seg[2].lda; ldw = a.seg[2].ldw;
            k0 = (s - st0n - st1n) * TBK;
        }
        return StageSrc{A + k0 + 4 * ldc4, W + k0 + 4 * ldc4, lda, ldw};
    };
    auto gpiece = [&](Regs& r, const StageSrc& ss, int piece) {
        if (piece < APASS) {
            const int row = min(piece * 32 + ldrow, a.M - 1);
            r.a[piece < APASS ? piece : 0] = ld4(ss.A + (size_t)row * ss.lda);
        } else if (piece < APASS + 2) {
            const int p = piece - APASS;
            const int row = min(n0 + p * 32 + ldrow, a.N - 1);
            r.w[p & 1] = ld4(ss.W + (size_t)row * ss.ldw);
        }
    };
    auto compute = [&](int buf, Regs* nx, int s_next) {
        const float* As = smem + buf * BUF;
        const float* Ws = As + AROWS * TLD + (wave * 16 + li) * TLD;
        StageSrc ss{};
        if (nx) ss = stage_src(s_next);
#pragma unroll
        for (int cc = 0; cc < TBK / 32; ++cc) {
            const int c = khalf * (TBK / 32) + cc;
            const float4 b = *reinterpret_cast<const float4*>(Ws + 16 * c + 4 * kk);
            float4 av[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t)
                av[t] = *reinterpret_cast<const float4*>(As + (t * 16 + li) * TLD + 16 * c + 4 * kk);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[t] = mfma16(comp(av[t], j), comp(b, j), acc[t]);
                if (nx) gpiece(*nx, ss, cc * 4 + j);             // 8 slots >= APASS + 2 pieces
            }
        }
    };

    // Two register sets alternate over two LDS buffers; the refill of a set (its six loads) is
    // interleaved with the MFMAs of the stage that follows its store.  Look-ahead: rb is loaded
    // during stage s and stored after stage s+1, ra during stage s+1 and stored after stage s+2.
    // Prefetch indices are clamped, not predicated.
    if (s_lo < s_hi) {
        const int last = s_hi - 1;
        Regs ra, rb;
        gload(ra, s_lo);
        lstore(ra, 0);
        gload(ra, min(s_lo + 1, last));
        gload(rb, min(s_lo + 2, last));
        __syncthreads();
        bool first = true;
        for (int s = s_lo; s < s_hi; s += 2) {
            compute(0, first ? nullptr : &rb, min(s + 2, last));   // stage s; rb <- s+2 (after the 1st)
            first = false;
            lstore(ra, 1);
            __syncthreads();
            if (s + 1 >= s_hi) break;
            compute(1, &ra, min(s + 3, last));                     // stage s+1; ra <- s+3
            lstore(rb, 0);
            __syncthreads();
        }
    }
    __syncthreads();

    // the two K halves meet in LDS (the stage buffers are free after the loop's last barrier)
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    if (khalf == 1) {
#pragma unroll
        for (int t = 0; t < MT; ++t) red[(wave * MT + t) * 64 + lane] = acc[t];
    }
    __syncthreads();
    if (khalf == 1) return;
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] += red[(wave * MT + t) * 64 + lane];

    const int col = n0 + wave * 16 + li;
    if (col >= a.N) return;
    float* out = a.out + (a.ksplit > 1 ? (size_t)split * a.M * a.N : 0);
    float bsum = 0.f;
    if (a.bias) bsum += a.bias[col];
    if (a.bias2) bsum += a.bias2[col];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + kk * 4 + r;
            if (row < a.M) {
                float* o = out + (size_t)row * a.ldo + col;
                const float v = acc[t][r] + bsum;
                *o = (a.accumulate && a.ksplit == 1) ? *o + v : v;
            }
        }
}

// ------------------------------------------------------------------------------------------------
// The same product on the BF16 matrix cores, at fp32 accuracy, by error-free operand splitting (round 4; the
// arithmetic, its error analysis and the measurements against float64 are in sf_split.h).  The gate product was the
// one MFMA-bound kernel of the path (fp32 MFMA loop at 92 % of the f32 vector rate); six bf16 MFMAs per product are
// 6/16 of that time, and what bounds the kernel now is moving its operands (timed with the MFMAs removed: 16 of its
// 20 us).
//
// Block = 64 columns x all rows (<= 128, as MT m-tiles of 16) x one K split; 8 waves = 4 n-tiles of 16
// columns x the 2 K-halves of every 64-deep stage -- the decomposition of gemm_nt_tiled_kernel, with
// v_mfma_f32_16x16x32_bf16 (one instruction per 32-deep half).  Operands are fetched as fp32 with full
// 256-B row segments (as the fp32 kernel does), split by the thread that fetched them and stored to LDS
// as three bf16 planes per operand ([row][64 k] = 128 B per row and plane, 16-B chunks XOR-swizzled with
// (row >> 1) & 7: the ds_read_b128 lane groups of gfx950 -- 16 rows, chunk c for 8 of them and c + 1 for
// the others -- then hit 16 distinct 16-B bank groups without padding: 2 x 3 x 176 rows x 128 B = 132 KB of
// the 160 KB at 112 rows).  The split + LDS stores of stage s+1 and the global loads of stage s+3 sit between
// the MFMAs of stage s: one barrier per stage.  The K halves meet in LDS as in the fp32 kernel.
// ------------------------------------------------------------------------------------------------
//
// BW (gemm_nt_bf16w_kernel, sf_gate_product_bf16_weights): the weight operand is ONE bf16 plane, rounded and packed once by
// pack_bf16_kernel -- half the bytes of the fp32 rows and no split in the loop.  The activation side is the same error-free
// three-way split, so a product is three MFMAs (a1 w into hi; a2 w, a3 w into lo) and equals the fp32-accurate product of
// the unrounded activations with bf16(W).  Everything else -- block shape, stages, K splits, prefetch ring, epilogue -- is
// the code below, shared.
// ------------------------------------------------------------------------------------------------
// (SPL_ROWB = 128 bytes per row and plane, 64 bf16: sf_gemm_plan.h)

// The packed bf16 weight image of one [rows, K] matrix (K % 64 == 0; rows padded with zeros to a multiple of 16):
// [n-tile of 16 rows][64-deep stage][K half][lane = 16 kk + li][8 bf16].  The 16 bytes of lane (li, kk) are what that lane
// feeds one v_mfma_f32_16x16x32_bf16 for row 16 tile + li: k = 32 half + 4 kk .. + 3 and 32 half + 16 + 4 kk .. + 3, the K
// order of the activation planes in LDS.  A wave's fragment of a stage is one global_load_dwordx4 over 1 KB of whole lines.
// (BW_STAGE_BYTES = 2 * 64 * 16 per n-tile and stage: sf_gemm_plan.h)
struct NtPackedW {
    const void* p[3];
};

template <int MT, bool BW>
__device__ __forceinline__ void nt_split_body(const NtArgs a, const NtPackedW pk) {   // (by value: the code of <MT, false> stays what it was as a kernel)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    constexpr int APASS = (MT + 1) / 2;                  // 32 rows x 16 float4 per staging pass
    constexpr int AROWS = APASS * 32;                    // (whole passes: every staging store is unconditional)
    constexpr int PLANE_A = AROWS * SPL_ROWB;
    constexpr int BUF = 3 * PLANE_A;                     // bytes per stage buffer (A only: W never touches LDS)
    constexpr int NW = BW ? 1 : 2;                       // 16-byte loads of a W fragment (8 bf16, or 8 fp32)
    constexpr int NPIECE = APASS + NW;                   // loads per thread and stage: APASS of A, NW of W
    const int tid = threadIdx.x, lane = tid & 63, wave8 = tid >> 6;
    const int wave = wave8 & 3, khalf = wave8 >> 2;      // n-tile of 16 columns, K-half of a stage
    const int li = lane & 15, kk = lane >> 4;
    int n0, split;
    {   // XCD-aware (split, n-block) map, as gemm_nt_tiled_kernel
        const int total = gridDim.x * gridDim.y;
        const int b = blockIdx.x + gridDim.x * blockIdx.y;
        int g = b;
        if ((total & 7) == 0) g = (b & 7) * (total >> 3) + (b >> 3);
        split = g / (int)gridDim.x;
        n0 = (g % (int)gridDim.x) * 64;
    }
    const int ldrow = tid >> 4, ldc4 = tid & 15;         // A staging: 32 rows x 16 float4 per pass
    const int st0n = a.seg[0].K / TBK;
    const int st1n = a.nseg > 1 ? a.seg[1].K / TBK : 0;
    const int st2n = a.nseg > 2 ? a.seg[2].K / TBK : 0;
    const int stages = st0n + st1n + st2n;
    const int s_lo = (int)(((long)split * stages) / a.ksplit);
    const int s_hi = (int)(((long)(split + 1) * stages) / a.ksplit);

    f32x4 hi[MT], lo[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) hi[t] = lo[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Staging registers are filled by INLINE-ASM loads and released by counted `s_waitcnt vmcnt(N)`: the compiler's own
    // bookkeeping loses the count across the loop's back edge and waits vmcnt(0) at the first use in every stage,
    // i.e. for the loads issued one stage earlier -- a prefetch distance of one stage (~1 us) against an HBM latency
    // of 1-2 us under load.  Loads return in order, so "at most N newer loads outstanding" means this one has landed.
    struct Regs {
        f32x4 a[APASS];          // A: this thread's float4 of rows 32 p + ldrow (shared through LDS)
        f32x4 w[NW];             // W: THIS WAVE's fragment rows (n-tile, K-half), never shared: registers only
    };
    struct StageSrc {
        const float* A;          // wave-uniform bases (SGPR pairs): the row offset travels in one VGPR
        const float* W;
        int lda, ldw;
    };
    // The segment of a stage is picked with mask arithmetic on values that sit in SGPRs: no branch (a stage's whole
    // body stays ONE basic block the scheduler can interleave), no load (a select of loaded values is turned into a
    // load from a selected address, i.e. a memory round trip at the head of every stage).
    // (BW: the W base is the segment's packed image and `ldw` its stage count -- the stride of an n-tile in stages)
    const unsigned long long pa0 = (unsigned long long)a.seg[0].A, pw0 = (unsigned long long)(BW ? pk.p[0] : a.seg[0].W),
                             pa1 = (unsigned long long)a.seg[1].A, pw1 = (unsigned long long)(BW ? pk.p[1] : a.seg[1].W),
                             pa2 = (unsigned long long)a.seg[2].A, pw2 = (unsigned long long)(BW ? pk.p[2] : a.seg[2].W);
    const unsigned lda0 = a.seg[0].lda, ldw0 = BW ? st0n : a.seg[0].ldw, lda1 = a.seg[1].lda, ldw1 = BW ? st1n : a.seg[1].ldw,
                   lda2 = a.seg[2].lda, ldw2 = BW ? st2n : a.seg[2].ldw;
    auto stage_src = [&](int s) {
        const unsigned long long m0 = s < st0n ? ~0ull : 0ull, m2 = s >= st0n + st1n ? ~0ull : 0ull, m1 = ~(m0 | m2);
        const int k0 = (s - (int)((unsigned)st0n & (unsigned)~m0) - (int)((unsigned)st1n & (unsigned)m2)) * TBK;
        return StageSrc{reinterpret_cast<const float*>((pa0 & m0) | (pa1 & m1) | (pa2 & m2)) + k0,
                        reinterpret_cast<const float*>((pw0 & m0) | (pw1 & m1) | (pw2 & m2)) +
                            (BW ? (BW_STAGE_BYTES / 4 / TBK) * k0 : k0),
                        (int)((lda0 & (unsigned)m0) | (lda1 & (unsigned)m1) | (lda2 & (unsigned)m2)),
                        (int)((ldw0 & (unsigned)m0) | (ldw1 & (unsigned)m1) | (ldw2 & (unsigned)m2))};
    };
    auto gld = [&](f32x4& dst, const float* base, unsigned byte_off) {
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(byte_off), "s"(base) : "memory");
    };
    // The K index inside one MFMA is free as long as A and B agree.  Lane (li, kk) holds, of its row's 32-deep half,
    // k = 4 kk .. 4 kk + 3 and 16 + 4 kk .. 16 + 4 kk + 3: a W fragment is then two 16-byte loads per lane whose 16-lane
    // groups read FULL 64-byte lines of a row (the straight 8-consecutive-k mapping reads half of every line twice).
    const int wrow = min(n0 + wave * 16 + li, a.N - 1);
    const int wtile = min((n0 >> 4) + wave, ((a.N + 15) >> 4) - 1);  // BW: this wave's n-tile of the packed image
    auto gpiece = [&](Regs& r, const StageSrc& ss, int piece) {       // one global load of the staging set
        if (piece < APASS) {
            const int row = min(piece * 32 + ldrow, a.M - 1);
            gld(r.a[piece < APASS ? piece : 0], ss.A, (unsigned)(row * ss.lda + 4 * ldc4) * 4u);
        } else if (piece < NPIECE) {
            const int e = piece - APASS;
            if constexpr (BW)
                gld(r.w[0], ss.W, (unsigned)(wtile * ss.ldw) * (unsigned)BW_STAGE_BYTES + (unsigned)(khalf * 64 + lane) * 16u);
            else
                gld(r.w[e & 1], ss.W, (unsigned)(wrow * ss.ldw + 32 * khalf + 16 * e + 4 * kk) * 4u);
        }
    };
    // piece `piece` of `r` has landed once at most `newer` younger loads are outstanding
#define SPL_LANDED(reg, newer) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(reg) : "n"(newer))
    // A planes in LDS: [plane][row][64 k bf16]; inside a row the 16-byte chunk (half g, lane group kk) holds
    // k = 32 g + 4 kk .. + 3 (first 8 bytes) and 32 g + 16 + 4 kk .. + 3 (last 8 bytes); chunks XOR-swizzled with (row >> 1) & 7
    auto st_off = [&](int row, int c4) {
        const int chunk = ((c4 >> 3) << 2) | (c4 & 3), e = (c4 >> 2) & 1;
        return row * SPL_ROWB + (((chunk ^ (row >> 1)) & 7) << 4) + (e << 3);
    };
    auto spiece_a = [&](const Regs& r, int buf, int piece) {          // split one float4 of A, three 8-byte LDS stores
        uint2 p1, p2, p3;
        const f32x4 v = r.a[piece < APASS ? piece : 0];
        split3_f4(make_float4(v[0], v[1], v[2], v[3]), p1, p2, p3);
        unsigned char* d = smem_b + buf * BUF + st_off(piece * 32 + ldrow, ldc4);
        *reinterpret_cast<uint2*>(d) = p1;
        *reinterpret_cast<uint2*>(d + PLANE_A) = p2;
        *reinterpret_cast<uint2*>(d + 2 * PLANE_A) = p3;
    };
    struct BFrag {
        bf16x8 p[BW ? 1 : 3];
    };
    auto split_w = [&](const Regs& r, BFrag& f) {                     // this wave's W fragment of the next stage
        if constexpr (BW) {
            // packed: the 16 bytes ARE the fragment -- but COPIED out of the staging register by instructions of their own.
            // A fragment that merely aliases it lets the register allocator give the reload (issued right behind this) a
            // fresh register and move that one into place at the loop's back edge, i.e. read it before its load has landed.
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float o;
                const float i = r.w[0][c];
                asm volatile("v_mov_b32 %0, %1" : "=v"(o) : "v"(i));
                v[c] = o;
            }
            f.p[0] = __builtin_bit_cast(bf16x8, v);
        } else {
            uint2 x1, x2, x3, y1, y2, y3;
            split3_f4(make_float4(r.w[0][0], r.w[0][1], r.w[0][2], r.w[0][3]), x1, x2, x3);
            split3_f4(make_float4(r.w[1][0], r.w[1][1], r.w[1][2], r.w[1][3]), y1, y2, y3);
            f.p[0] = __builtin_bit_cast(bf16x8, uint4{x1.x, x1.y, y1.x, y1.y});
            f.p[1] = __builtin_bit_cast(bf16x8, uint4{x2.x, x2.y, y2.x, y2.y});
            f.p[2] = __builtin_bit_cast(bf16x8, uint4{x3.x, x3.y, y3.x, y3.y});
        }
    };
    const int fchunk = 4 * khalf + kk;
    auto frag = [&](const unsigned char* plane, int row) {
        return *reinterpret_cast<const bf16x8*>(plane + row * SPL_ROWB + (((fchunk ^ (row >> 1)) & 7) << 4));
    };
    // One stage: 6 MT (BW: 3 MT) MFMAs on buffer `buf` with the W fragment `bc`.  `rs` holds the raw operands of the NEXT stage:
    // its A pieces are split into LDS buffer `sbuf`, its W pieces into the fragment `bn`, and every register is
    // reloaded with its piece of stage `s_next` right behind its use.
    auto compute = [&](int buf, const BFrag& bc, Regs& rs, BFrag& bn, int s_next, int sbuf) {
        const unsigned char* Ab = smem_b + buf * BUF;
        const StageSrc ss = stage_src(s_next);
        // the staging work of slot t (between the MFMAs of tile t)
        auto stage_work_a = [&](int t) {
            if (t < APASS) {
                // younger than this piece's load: the other set's NPIECE loads of the previous stage and this set's t
                // reloads of this stage
                SPL_LANDED(rs.a[t < APASS ? t : 0], NPIECE + t);
                spiece_a(rs, sbuf, t);
            } else if (t == APASS) {
                SPL_LANDED(rs.w[0], NPIECE + APASS);
                SPL_LANDED(rs.w[NW - 1], NPIECE + APASS);
                split_w(rs, bn);
            }
        };
        auto stage_work_b = [&](int t) {
            if (t < APASS) gpiece(rs, ss, t);
            else if (t == APASS) { gpiece(rs, ss, APASS); gpiece(rs, ss, APASS + 1); }   // (BW: piece APASS + 1 does not exist)
        };
        // Tiles go in PAIRS with their MFMAs interleaved (consecutive MFMAs never share an accumulator) and the
        // fragments of the next pair are requested before the current pair's MFMAs are issued.
        bf16x8 fa[2][2][3];                                           // [parity][tile of the pair][plane]
        auto fetch = [&](int pr, int t0) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (t0 + u < MT) {
                    const int arow = (t0 + u) * 16 + li;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) fa[pr][u][pl] = frag(Ab + pl * PLANE_A, arow);
                }
        };
        fetch(0, 0);
#pragma unroll
        for (int t0 = 0; t0 < MT; t0 += 2) {
            const int pr = (t0 >> 1) & 1;
            if (t0 + 2 < MT) fetch(pr ^ 1, t0 + 2);
            const bool two = t0 + 1 < MT;
            const int t1 = two ? t0 + 1 : t0;
#define SPL_MM(acc, t, pa, pb) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[pr][(t) - t0][pa], bc.p[pb], acc[t], 0, 0, 0)
            SPL_MM(lo, t0, 2, 0);
            if (two) SPL_MM(lo, t1, 2, 0);
            if constexpr (!BW) {
                SPL_MM(lo, t0, 0, 2);
                if (two) SPL_MM(lo, t1, 0, 2);
            }
            stage_work_a(t0);
            if constexpr (!BW) {
                SPL_MM(lo, t0, 1, 1);
                if (two) SPL_MM(lo, t1, 1, 1);
            }
            SPL_MM(lo, t0, 1, 0);
            if (two) SPL_MM(lo, t1, 1, 0);
            stage_work_b(t0);
            if (two) stage_work_a(t1);
            if constexpr (!BW) {
                SPL_MM(lo, t0, 0, 1);
                if (two) SPL_MM(lo, t1, 0, 1);
            }
            SPL_MM(hi, t0, 0, 0);
            if (two) SPL_MM(hi, t1, 0, 0);
            if (two) stage_work_b(t1);
#undef SPL_MM
        }
        if (MT <= APASS) {                                            // (MT = 1: the W pieces did not fit above)
            SPL_LANDED(rs.w[0], NPIECE + APASS);
            SPL_LANDED(rs.w[NW - 1], NPIECE + APASS);
            split_w(rs, bn);
            gpiece(rs, ss, APASS);
            gpiece(rs, ss, APASS + 1);
        }
    };
    auto gload = [&](Regs& r, int s) {
        const StageSrc ss = stage_src(s);
#pragma unroll
        for (int piece = 0; piece < NPIECE; ++piece) gpiece(r, ss, piece);
    };

    // Register sets ra / rb alternate: at the top of stage s the buffer of s holds its A planes and one fragment its W
    // pieces; one set holds the raw operands of stage s+1 (landed) and the other those of stage s+2 (in flight).
    // Stage indices are clamped, not predicated.
    if (s_lo < s_hi) {
        const int last = s_hi - 1;
        Regs ra, rb;
        BFrag b0, b1;
        gload(ra, s_lo);
        gload(rb, min(s_lo + 1, last));
#pragma unroll
        for (int piece = 0; piece < APASS; ++piece) {
            SPL_LANDED(ra.a[piece], NPIECE);                          // (rb's loads are younger)
            spiece_a(ra, 0, piece);
        }
        SPL_LANDED(ra.w[0], NPIECE);
        SPL_LANDED(ra.w[NW - 1], NPIECE);
        split_w(ra, b0);
        gload(ra, min(s_lo + 2, last));
        __syncthreads();
        for (int s = s_lo; s < s_hi; s += 2) {
            compute(0, b0, rb, b1, min(s + 3, last), 1);      // stage s on buffer 0; rb (s+1) -> buffer 1 / b1; rb <- s+3
            __syncthreads();
            if (s + 1 >= s_hi) break;
            compute(1, b1, ra, b0, min(s + 4, last), 0);      // stage s+1 on buffer 1; ra (s+2) -> buffer 0 / b0; ra <- s+4
            __syncthreads();
        }
    }
    // (the clamped prefetches of the last stages are still in flight: nothing below may reuse their registers yet)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#undef SPL_LANDED

    // the two K halves meet in LDS (the stage buffers are free behind the loop's last barrier)
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = hi[t] + lo[t];
    f32x4* red = reinterpret_cast<f32x4*>(smem_b);
    if (khalf == 1) {
#pragma unroll
        for (int t = 0; t < MT; ++t) red[(wave * MT + t) * 64 + lane] = acc[t];
    }
    __syncthreads();
    if (khalf == 1) return;
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] += red[(wave * MT + t) * 64 + lane];

    const int col = n0 + wave * 16 + li;
    if (col >= a.N) return;
    float* out = a.out + (a.ksplit > 1 ? (size_t)split * a.M * a.N : 0);
    float bsum = 0.f;
    if (a.bias) bsum += a.bias[col];
    if (a.bias2) bsum += a.bias2[col];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + kk * 4 + r;
            if (row < a.M) {
                float* o = out + (size_t)row * a.ldo + col;
                const float v = acc[t][r] + bsum;
                *o = (a.accumulate && a.ksplit == 1) ? *o + v : v;
            }
        }
}

template <int MT>
__global__ __launch_bounds__(512) void gemm_nt_split_kernel(NtArgs a) {
    nt_split_body<MT, false>(a, NtPackedW{});
}

template <int MT>
__global__ __launch_bounds__(512) void gemm_nt_bf16w_kernel(NtArgs a, NtPackedW pk) {
    nt_split_body<MT, true>(a, pk);
}

// fp32 [rows, K] (leading dimension ld) -> the packed bf16 image above: one thread per lane fragment (two float4 in,
// 16 bytes out).  Round to nearest even on the bit pattern, the arithmetic of torch's float -> bfloat16 conversion
// (subnormals are rounded like any other value, a NaN becomes the quiet NaN 0x7FC0); rows past `rows` are zeros.
__device__ __forceinline__ unsigned bf16_rne_bits(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ w, int ld, int rows, int K,
                                                        uint4* __restrict__ out, unsigned total) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;      // = ((tile * stages + stage) * 2 + half) * 64 + lane
    if (i >= total) return;
    const unsigned lane = i & 63u, half = (i >> 6) & 1u, ts = i >> 7;
    const unsigned stages = (unsigned)K / TBK, tile = ts / stages, stage = ts % stages;
    const unsigned row = tile * 16u + (lane & 15u), k = stage * TBK + half * 32u + 4u * (lane >> 4);
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (row < (unsigned)rows) {
        const float* src = w + (size_t)row * ld + k;
        const float4 x = ld4(src), y = ld4(src + 16);
        o.x = bf16_rne_bits(x.x) | (bf16_rne_bits(x.y) << 16);
        o.y = bf16_rne_bits(x.z) | (bf16_rne_bits(x.w) << 16);
        o.z = bf16_rne_bits(y.x) | (bf16_rne_bits(y.y) << 16);
        o.w = bf16_rne_bits(y.z) | (bf16_rne_bits(y.w) << 16);
    }
    out[i] = o;
}

// ------------------------------------------------------------------------------------------------
// MANY-ROW NT product (round 5): C[M,N] = A[M,K] W[N,K]^T (+ bias, + addend, tanh) for M >= 512 -- the speaker's
// teacher-forced head over all S*B = 8 000 rows (t_text, h~, vocabulary projection and their data gradients), the beam
// search's flat decoder steps over 2 560 states.  gemm_nt_kernel streams its operands straight from global memory (7
// FLOPs per operand byte: 38-55 TFLOP/s at M = 8 000); here a workgroup forms a 128 x 128 tile from 32-deep stages of
// both operands staged through LDS as three bf16 planes each (error-free three-way split, sf_split.h: fp32 accuracy on
// the bf16 matrix cores, 32 FLOPs per operand byte).  512 threads = 2 x 4 waves of 64 x 32 outputs (8 MFMA tiles, hi / lo
// accumulators); per stage a thread fetches 2 + 2 float4, splits them once and stores 12 x 8 bytes; double-buffered LDS
// (96 KB), the next stage's global loads in flight under the current stage's 48 MFMAs per wave; one barrier per stage.
// Row layout of a plane: 64 bytes per row and stage = four 16-byte chunks, chunk kk = {k = 4 kk .. +3 | 16 + 4 kk .. +3}:
// what one lane feeds one v_mfma_f32_16x16x32_bf16 (the K order inside an MFMA is free as long as A and B agree).
// ------------------------------------------------------------------------------------------------
struct NtBigArgs {
    Seg seg[3];            // up to three K segments ([x | h] W = x W_x + h W_h: the LSTM gates); K_s % 4 == 0
    int nseg;
    int M, N;
    float* y; int ldy;
    const float* bias; const float* bias2;
    const float* addend; int ld_addend;
    int epi, accumulate;
    int ksplit;            // > 1: grid.y K-splits, split z writes its partial tile to slab y + z * M * N (ldy = N, plain)
};
// (NB_T = 128, NB_K = 32, NB_PLANE = NB_T * 64 bytes per plane and stage, 128 rows x 64 B: sf_gemm_plan.h)

__device__ __forceinline__ void nt_big_body(const NtBigArgs& a, const int tile, const int split_of_block) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nb_smem[];   // [2 buffers][A | W][3 planes][128 rows][64 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int wm = wave >> 2, wn = wave & 3;                          // 64-row half, 32-column quarter of the tile
    // tile map (XCD-aware): workgroup b runs on XCD b % 8, each XCD with its own L2.  XCD x takes a CONTIGUOUS run of the
    // tiles in column-fastest order, so the column blocks that share a 128-row slice of A are co-resident on one XCD and
    // stream it through one L2 (before: rows-fastest over all XCDs, every slice of A fetched once per column block from
    // beyond the L2s).  Measured with the bank swizzle below: +2 .. +6 % (profiles/r05_zz_many_row_kernel_lab.txt).
    const int mtiles = (a.M + NB_T - 1) / NB_T, ntiles = (a.N + NB_T - 1) / NB_T;
    const int tiles_all = mtiles * ntiles, xcd = tile & 7;
    const int order = xcd * (tiles_all >> 3) + min(xcd, tiles_all & 7) + (tile >> 3);
    const int m0 = (order / ntiles) * NB_T, n0 = (order % ntiles) * NB_T;
    // staging: thread -> (row = tid >> 3 (+64), float4 c4 = tid & 7 of the 32-deep stage)
    const int srow = tid >> 3, c4 = tid & 7;
    int arow[2], wrow[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        arow[p] = min(m0 + srow + 64 * p, a.M - 1);
        wrow[p] = min(n0 + srow + 64 * p, a.N - 1);
    }
    const int st0 = (a.seg[0].K + NB_K - 1) / NB_K, st1 = a.nseg > 1 ? (a.seg[1].K + NB_K - 1) / NB_K : 0,
              st2 = a.nseg > 2 ? (a.seg[2].K + NB_K - 1) / NB_K : 0;
    // stage s -> its segment and depth offset (wave-uniform selects); a segment's last stage may be partial (K_s % 4 == 0):
    // loads beyond K_s are clamped and replaced by zeros
    auto gload = [&](int s, float4 (&ra)[2], float4 (&rw)[2]) {
        const int g = s < st0 ? 0 : (s < st0 + st1 ? 1 : 2);
        const int k0 = (s - (g > 0 ? st0 : 0) - (g > 1 ? st1 : 0)) * NB_K + 4 * c4;
        const Seg& sg = a.seg[g];
        const bool ok = k0 < sg.K;
        const int kc = ok ? k0 : 0;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float4 x = ld4(sg.A + (size_t)arow[p] * sg.lda + kc), y = ld4(sg.W + (size_t)wrow[p] * sg.ldw + kc);
            ra[p] = ok ? x : z;
            rw[p] = ok ? y : z;
        }
    };
    // Bank swizzle: a ds_read_b128 is served in groups of 16 lanes over 64 banks, and rows r, r + 4, r + 8, r + 12 of a
    // 64-byte-row plane start on the same bank: chunk kk of row r lives at position kk ^ ((-(r >> 2)) & 3), which gives the
    // four rows of every lane group four different chunk positions (unswizzled: 2-way conflicts, 8 instead of 4 LDS cycles
    // per fragment read).  srow, srow + 64 and the fragment rows 16 i + li all have (row >> 2) & 3 from their low bits.
    const int soff = srow * 64 + ((((c4 & 3) ^ (-(srow >> 2))) & 3) << 4) + ((c4 >> 2) << 3);   // this thread's 8 bytes inside a plane
    auto stage_store = [&](int buf, const float4 (&ra)[2], const float4 (&rw)[2]) {
        unsigned char* base = nb_smem + buf * (6 * NB_PLANE);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            uint2 p1, p2, p3;
            split3_f4(ra[p], p1, p2, p3);
            unsigned char* d = base + soff + p * 64 * 64;
            *reinterpret_cast<uint2*>(d) = p1;
            *reinterpret_cast<uint2*>(d + NB_PLANE) = p2;
            *reinterpret_cast<uint2*>(d + 2 * NB_PLANE) = p3;
            split3_f4(rw[p], p1, p2, p3);
            d += 3 * NB_PLANE;
            *reinterpret_cast<uint2*>(d) = p1;
            *reinterpret_cast<uint2*>(d + NB_PLANE) = p2;
            *reinterpret_cast<uint2*>(d + 2 * NB_PLANE) = p3;
        }
    };
    f32x4 hi[4][2], lo[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) hi[i][j] = lo[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int stages_all = st0 + st1 + st2;
    const int ks = a.ksplit > 1 ? a.ksplit : 1, split = split_of_block;
    const int s_lo = (int)(((long)split * stages_all) / ks), s_hi = (int)(((long)(split + 1) * stages_all) / ks);
    const int stages = s_hi - s_lo;
    // Two register sets: the loads of stage s + 2 are issued at the top of stage s and stored to LDS at the end of stage
    // s + 1 -- two stages (~1.2 us) of latency hiding; one stage is less than an HBM round trip under load.
    float4 ra[2][2], rw[2][2];
    auto compute = [&](int buf) {
        const int kpos = ((kk ^ (-(li >> 2))) & 3) * 16;
        const unsigned char* Ab = nb_smem + buf * (6 * NB_PLANE) + (wm * 64 + li) * 64 + kpos;
        const unsigned char* Wb = nb_smem + buf * (6 * NB_PLANE) + 3 * NB_PLANE + (wn * 32 + li) * 64 + kpos;
        Split8 wf[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) wf[j].p[pl] = *reinterpret_cast<const bf16x8*>(Wb + pl * NB_PLANE + j * 16 * 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Split8 af;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) af.p[pl] = *reinterpret_cast<const bf16x8*>(Ab + pl * NB_PLANE + i * 16 * 64);
            mfma_split6_across<2>(af, [&](int j) -> const Split8& { return wf[j]; }, hi[i], lo[i]);
        }
    };
    const int last = s_hi - 1;
    gload(s_lo, ra[0], rw[0]);
    stage_store(0, ra[0], rw[0]);
    gload(min(s_lo + 1, last), ra[1], rw[1]);                        // set 1 <- stage 1 (in flight during stage 0)
    __syncthreads();
    for (int s = 0; s < stages; s += 2) {
        gload(min(s_lo + s + 2, last), ra[0], rw[0]);                 // set 0 <- stage s + 2
        compute(0);
        if (s + 1 < stages) stage_store(1, ra[1], rw[1]);             // stage s + 1 (issued one stage ago) -> buffer 1
        __syncthreads();
        if (s + 1 >= stages) break;
        gload(min(s_lo + s + 3, last), ra[1], rw[1]);                 // set 1 <- stage s + 3
        compute(1);
        if (s + 2 < stages) stage_store(0, ra[0], rw[0]);             // stage s + 2 -> buffer 0
        __syncthreads();
    }
    // epilogue: lane (li, kk) holds rows 4 kk + r, column li of every 16 x 16 tile
    if (ks > 1) {                                                     // K-split: the plain partial tile into this split's slab
        float* slab = a.y + (size_t)split * a.M * a.N;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 32 + j * 16 + li;
            if (col >= a.N) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = m0 + wm * 64 + i * 16 + kk * 4 + r;
                    if (row < a.M) slab[(size_t)row * a.N + col] = hi[i][j][r] + lo[i][j][r];
                }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 32 + j * 16 + li;
        if (col >= a.N) continue;
        float bsum = 0.f;
        if (a.bias) bsum += a.bias[col];
        if (a.bias2) bsum += a.bias2[col];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + i * 16 + kk * 4 + r;
                if (row >= a.M) continue;
                float v = (hi[i][j][r] + lo[i][j][r]) + bsum;
                if (a.addend) v += a.addend[(size_t)row * a.ld_addend + col];
                if (a.epi == EPI_TANH) v = tanhf(v);
                float* o = a.y + (size_t)row * a.ldy + col;
                *o = a.accumulate ? *o + v : v;
            }
    }
}

__global__ __launch_bounds__(512) void gemm_nt_big_kernel(NtBigArgs a) { nt_big_body(a, blockIdx.x, blockIdx.y); }

// SEVERAL many-row products in one launch (gemm_tn_group: the decoder's small weight gradients -- each a few dozen tiles,
// 35 dependent launches of 5-28 us between them when issued one by one): block b belongs to job j with
// first[j] <= b < first[j + 1]; inside the job blocks walk its tiles, then its K splits.
struct NtBigGroup {
    NtBigArgs job[NB_GROUP];
    int first[NB_GROUP + 1];
    int n;
};
__global__ __launch_bounds__(512) void gemm_nt_big_group_kernel(NtBigGroup g) {
    int j = 0;
#pragma unroll
    for (int k = 1; k < NB_GROUP; ++k) j += (k < g.n && (int)blockIdx.x >= g.first[k]) ? 1 : 0;
    const NtBigArgs& a = g.job[j];
    const int local = (int)blockIdx.x - g.first[j];
    const int tiles = ((a.M + NB_T - 1) / NB_T) * ((a.N + NB_T - 1) / NB_T);
    nt_big_body(a, local % tiles, local / tiles);
}

// Several transposes in one launch: problem p's 32 x 32 tiles are blocks first[p] .. first[p + 1] - 1
struct TrGroup {
    struct P { const float* src; float* dst; int lds, R, C; } p[TR_GROUP];
    int first[TR_GROUP + 1];
    int n;
};
__global__ __launch_bounds__(256) void transpose_group_kernel(TrGroup g) {
    __shared__ float tile[32][33];
    int j = 0;
#pragma unroll
    for (int k = 1; k < TR_GROUP; ++k) j += (k < g.n && (int)blockIdx.x >= g.first[k]) ? 1 : 0;
    const TrGroup::P q = g.p[j];
    const int local = (int)blockIdx.x - g.first[j], ct = (q.C + 31) / 32;
    const int c0 = (local % ct) * 32, r0 = (local / ct) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < q.R && c0 + tx < q.C) tile[i][tx] = q.src[(size_t)(r0 + i) * q.lds + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < q.C && r0 + tx < q.R) q.dst[(size_t)(c0 + i) * q.R + r0 + tx] = tile[tx][i];
}

// out_j (+)= sum of job j's K-split slabs, all jobs in one launch (grid.y = job; fixed slab order: deterministic)
struct RedGroup {
    struct J { const float* slabs; float* y; int ks, M, N, ldy, accumulate; } j[NB_GROUP];
};
__global__ __launch_bounds__(256) void reduce_slabs_group_kernel(RedGroup g) {
    const RedGroup::J a = g.j[blockIdx.y];
    const size_t total = (size_t)a.M * a.N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / a.N), col = (int)(i % a.N);
        float v = 0.f;
        for (int s = 0; s < a.ks; ++s) v += a.slabs[(size_t)s * total + i];
        float* o = a.y + (size_t)row * a.ldy + col;
        *o = a.accumulate ? *o + v : v;
    }
}

// ------------------------------------------------------------------------------------------------
// Short reductions (K <= 1024: every Linear of the decode step except the LSTM gates, and the
// recurrent h*W_hh^T of the encoder / speaker decoder).  These are LATENCY bound: a wave that walks
// its K range chunk by chunk pays one HBM round trip per chunk (measured 13 us for K = 512).  So the
// K range of one output tile is split over the waves of the block, every wave issues ALL its loads
// before the first MFMA (<= CPW chunks of (1 + MT) float4 per lane), and the partial tiles meet in
// LDS where the epilogue runs: one HBM round trip per launch, no split-K slabs, no second kernel.
// ------------------------------------------------------------------------------------------------
// (Seg2, Frags, upfront_load / upfront_mma, SmallArgs and the kernel body live in sf_gemm_small.h:
// the paired launches of sf_attention.hip run the same body next to an attention body.)
template <int MT, int CPW>
__global__ __launch_bounds__(SMALL_WAVES * 64) void gemm_nt_small_kernel(SmallArgs a) {
    small_gemm_body<MT, CPW>(a, blockIdx.x, blockIdx.y);
}
template <int MT, int CPW>     // with the fused backward epilogues (see small_gemm_body)
__global__ __launch_bounds__(SMALL_WAVES * 64) void gemm_nt_small_x_kernel(SmallArgs a) {
    small_gemm_body<MT, CPW, true>(a, blockIdx.x, blockIdx.y);
}

// Fused recurrent LSTM step (nn.LSTMCell / one nn.LSTM time step): block = 16 waves = the 4 gate
// tiles (i,f,g,o) of one 16-row x 16-hidden-unit patch x 4 K-slices; gates meet in LDS and the cell
// update happens in the same kernel: ONE launch per time step.  grid (H/16, ceil(B/16)).
constexpr int LSTM_KS = 4;

template <int CPW>
__global__ __launch_bounds__(4 * LSTM_KS * 64) void lstm_step_fused_kernel(LstmStepArgs p) {
    __shared__ float s_g[4][LSTM_KS][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gate = wave & 3, ksl = wave >> 2;
    const int slice = blockIdx.x, m0 = blockIdx.y * 16;
    const int li = lane & 15, kk = lane >> 4;
    const int H = p.H;

    // tail operands (hoisted input product, biases) are fetched FIRST: xg[t] is a cold HBM read and
    // would otherwise sit, fully exposed, between the LDS reduction and the cell update
    const int prow = threadIdx.x >> 4, pcol = threadIdx.x & 15;
    const int pb = m0 + prow, pj = slice * 16 + pcol;
    const bool ptail = threadIdx.x < 256 && pb < p.B;
    float pre[4] = {0.f, 0.f, 0.f, 0.f};
    float c0v = 0.f;
    LstmLive lv{true, 0.f};
    {   // straight-line: rows / threads outside the tail read a clamped (valid) address
        const int qb = min(pb, p.B - 1);
        c0v = p.pw.c0[qb * H + pj];
        lv = lstm_live_load(p.pw, qb, pj);
        float bi[4], bh[4], xv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bi[g] = p.b_ih[g * H + pj];
            bh[g] = p.b_hh[g * H + pj];
        }
        if (p.xg) {                                              // block-uniform
            const size_t xr = p.xg_index ? (size_t)p.xg_index[(size_t)qb * max(p.xg_index_ld, 1)] : (size_t)qb;
#pragma unroll
            for (int g = 0; g < 4; ++g) xv[g] = p.xg[xr * 4 * H + g * H + pj];
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = bi[g] + bh[g] + xv[g];
        if (p.xg2) {                                             // block-uniform
#pragma unroll
            for (int g = 0; g < 4; ++g) pre[g] += p.xg2[(size_t)qb * 4 * H + g * H + pj];
        }
    }

    Seg2 sg;
    sg.s0 = Seg{p.h0, H, p.w_hh, H, H};
    sg.n0 = (H + 15) >> 4;
    sg.s1 = p.x ? Seg{p.x, p.ldx, p.w_ih, p.ld_w_ih ? p.ld_w_ih : p.I, p.I} : sg.s0;
    sg.total = sg.n0 + (p.x ? ((p.I + 15) >> 4) : 0);
    const int n = gate * H + slice * 16 + li;
    int mrow[1] = {min(m0 + li, p.B - 1)};
    const int c_lo = (ksl * sg.total) / LSTM_KS, c_hi = ((ksl + 1) * sg.total) / LSTM_KS;
    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    if (c_hi > c_lo) {
        Frags<1, CPW> f;
        upfront_load<1, CPW>(f, sg, c_lo, c_hi, n, mrow, kk);
        upfront_mma<1, CPW>(f, c_hi - c_lo, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) s_g[gate][ksl][(kk * 4 + r) * 16 + li] = acc[0][r];
    __syncthreads();

    if (!ptail) return;
    float g4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v = pre[g];
#pragma unroll
        for (int k = 0; k < LSTM_KS; ++k) v += s_g[g][k][threadIdx.x];
        g4[g] = v;
    }
    lstm_cell_update(p.pw, pb, pj, g4, c0v, lv);
}

// The same step with a 32-row x 8-hidden-unit patch per block (B > 16).  A recurrent step is bound by
// the bytes ONE block pulls through its CU (timestamped: the loads of the 16 x 16 patch -- 128 KB of
// W_hh, the 32 KB of h fetched once per gate wave = 256 KB issued -- keep landing for ~6 us of an
// 11.5 us step; the MFMAs take 1.7 us).  Per block the bytes are (4 hu + rows) x 2 KB, smallest at
// rows = 4 hu: 8 units x 32 rows = 128 KB, and with the 16 waves as 16 K-slices that each hold both
// m-tiles and both n-tiles nothing is fetched twice.  grid (H/8, ceil(B/32)).
//   n-tile q = gates (2q, 2q+1) x 8 units: column li -> W_hh row (2q + li/8) H + 8 slice + li%8.
constexpr int LSTMW_WAVES = 16;

template <int CPW>
__global__ __launch_bounds__(LSTMW_WAVES * 64) void lstm_step_wide_kernel(LstmStepArgs p) {
    __shared__ float s_red[LSTMW_WAVES / 2][4][256];     // 32 KB: partial tiles (t, q) of 8 waves
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.x, m0 = blockIdx.y * 32;
    const int li = lane & 15, kk = lane >> 4;
    const int H = p.H;

    // Tail operands.  The block updates 256 (row, unit) elements (threads 0..255 do it); their gate
    // biases and hoisted input rows are 12 scattered dword loads per element -- issued by all 1024
    // threads for their own element they were more vector-memory instructions than the fragments
    // (and ahead of them in the queue).  Instead thread (g, e) fetches gate g of element e: 4 loads,
    // the sums meet in LDS with the partial tiles.
    __shared__ float s_pre[4][256];
    const int pe = threadIdx.x & 255, pg = threadIdx.x >> 8;
    const int prow = pe >> 3, pcol = pe & 7;
    const int pb = m0 + prow, pj = slice * 8 + pcol;
    const bool ptail = threadIdx.x < 256 && pb < p.B;
    const int qb = min(pb, p.B - 1);
    float pre_g;
    {   // straight-line: rows outside the batch read a clamped (valid) address
        const float bi = p.b_ih[pg * H + pj], bh = p.b_hh[pg * H + pj];
        float xv = 0.f;
        if (p.xg) {                                              // block-uniform
            const size_t xr = p.xg_index ? (size_t)p.xg_index[(size_t)qb * max(p.xg_index_ld, 1)] : (size_t)qb;
            xv = p.xg[xr * 4 * H + pg * H + pj];
        }
        pre_g = bi + bh + xv;
        if (p.xg2) pre_g += p.xg2[(size_t)qb * 4 * H + pg * H + pj];      // block-uniform
    }

    // this wave's K-slice of all four tiles: every fragment is loaded before the first MFMA
    const int n0c = H >> 4;
    const int total = n0c + (p.x ? ((p.I + 15) >> 4) : 0);
    const int c_lo = (wave * total) / LSTMW_WAVES, c_hi = ((wave + 1) * total) / LSTMW_WAVES;
    const int nrow[2] = {(li >> 3) * H + slice * 8 + (li & 7), (2 + (li >> 3)) * H + slice * 8 + (li & 7)};
    const int mrow[2] = {min(m0 + li, p.B - 1), min(m0 + 16 + li, p.B - 1)};
    float4 fa[CPW][2], fb[CPW][2];
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int c = min(min(c_lo + i, max(c_hi - 1, c_lo)), total - 1);   // clamped: surplus slots re-load a valid chunk
        const bool second = c >= n0c;                            // wave-uniform
        const int lc = second ? c - n0c : c;
        const float* W = second ? p.w_ih : p.w_hh;
        const float* A = second ? p.x : p.h0;
        const int ldw = second ? (p.ld_w_ih ? p.ld_w_ih : p.I) : H;
        const int lda = second ? p.ldx : H;
        const int K = second ? p.I : H;
        const int k = lc * 16 + 4 * kk;
        const bool ok = k < K && c_lo + i < c_hi;                // partial last chunk / surplus slot
        const int kc = k < K ? k : 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 bv = ld4(W + (size_t)nrow[q] * ldw + kc);
            fb[i][q] = ok ? bv : z;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float4 av = ld4(A + (size_t)mrow[t] * lda + kc);
            fa[i][t] = ok ? av : z;
        }
    }
    // state operands of the tail threads (waves 0-3), behind the fragment loads in the queue
    float c0v = 0.f;
    LstmLive lv{true, 0.f};
    if (threadIdx.x < 256) {                                     // wave-uniform
        c0v = p.pw.c0[qb * H + pj];
        lv = lstm_live_load(p.pw, qb, pj);
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < CPW; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    acc[t][q] = mfma16(comp(fa[i][t], c), comp(fb[i][q], c), acc[t][q]);

    s_pre[pg][pe] = pre_g;
    // 16 partial tile sets -> 8 (through LDS) -> the cell update sums the 8
    if (wave >= LSTMW_WAVES / 2) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    s_red[wave - LSTMW_WAVES / 2][t * 2 + q][(kk * 4 + r) * 16 + li] = acc[t][q][r];
    }
    __syncthreads();
    if (wave < LSTMW_WAVES / 2) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float* sp = &s_red[wave][t * 2 + q][(kk * 4 + r) * 16 + li];
                    *sp += acc[t][q][r];                          // (same thread wrote / reads this slot)
                }
    }
    __syncthreads();

    if (!ptail) return;
    float g4[4];
    const int tt = prow >> 4, rr = prow & 15;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v = s_pre[g][pe];
        const int e = rr * 16 + (g & 1) * 8 + pcol;
#pragma unroll
        for (int k = 0; k < LSTMW_WAVES / 2; ++k) v += s_red[k][tt * 2 + (g >> 1)][e];
        g4[g] = v;
    }
    lstm_cell_update(p.pw, pb, pj, g4, c0v, lv);
}

// The decoder's step with its recurrent half as a row (LstmRowsArgs): what is left of the product is K <= 256 columns
// of x (the attended feature's location part, K = 128), so the same 32-row x 8-unit patch takes 8 waves = 8 K-slices of
// <= CPW chunks, and the block's bytes are the three [32 rows, 4 gates, 8 units] row patches: 32-byte runs along the gate
// row, one float4 per thread of waves 4-7 per row, while waves 0-3 (the tail threads) fetch the state.
// grid (H/8, ceil(B/32)).  Tile layout, partial-tile exchange and tail as in lstm_step_wide_kernel.
constexpr int LSTMR_WAVES = 8;

template <int CPW>
__global__ __launch_bounds__(LSTMR_WAVES * 64) void lstm_step_rows_kernel(LstmRowsArgs p) {
    __shared__ float s_red[LSTMR_WAVES][4][256];         // 32 KB: partial tiles (t, q) of the 8 waves
    __shared__ float s_pre[4][256];                      // the three rows summed: [gate][row * 8 + unit]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.x, m0 = blockIdx.y * 32;
    const int li = lane & 15, kk = lane >> 4;
    const int H = p.H;

    // rows: thread 256 + e4 holds float4 e4 of the patch: row e4 / 8, gate (e4 / 2) % 4, units 4 (e4 % 2) .. + 3
    const int e4 = threadIdx.x & 255;
    const int r_row = e4 >> 3, r_gate = (e4 >> 1) & 3, r_half = e4 & 1;
    float4 pre4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x >= 256) {                                    // wave-uniform; rows outside the batch read a clamped address
        const size_t off = (size_t)min(m0 + r_row, p.B - 1) * 4 * H + r_gate * H + slice * 8 + r_half * 4;
        const float4 a = ld4(p.xg_h + off), b = ld4(p.xg + off), c = ld4(p.xg2 + off);
        pre4 = make_float4((a.x + b.x) + c.x, (a.y + b.y) + c.y, (a.z + b.z) + c.z, (a.w + b.w) + c.w);
    }

    // this wave's K-slice of all four tiles: every fragment is loaded before the first MFMA
    const int total = (p.K + 15) >> 4;
    const int c_lo = (wave * total) / LSTMR_WAVES, c_hi = ((wave + 1) * total) / LSTMR_WAVES;
    const int nrow[2] = {(li >> 3) * H + slice * 8 + (li & 7), (2 + (li >> 3)) * H + slice * 8 + (li & 7)};
    const int mrow[2] = {min(m0 + li, p.B - 1), min(m0 + 16 + li, p.B - 1)};
    float4 fa[CPW][2], fb[CPW][2];
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int c = min(min(c_lo + i, max(c_hi - 1, c_lo)), total - 1);   // clamped: surplus slots re-load a valid chunk
        const int k = c * 16 + 4 * kk;
        const bool ok = k < p.K && c_lo + i < c_hi;              // partial last chunk / surplus slot / idle wave
        const int kc = k < p.K ? k : 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 bv = ld4(p.w + (size_t)nrow[q] * p.ldw + kc);
            fb[i][q] = ok ? bv : z;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float4 av = ld4(p.x + (size_t)mrow[t] * p.ldx + kc);
            fa[i][t] = ok ? av : z;
        }
    }
    // state operands of the tail threads (waves 0-3)
    const int prow = e4 >> 3, pcol = e4 & 7;
    const int pb = m0 + prow, pj = slice * 8 + pcol;
    const bool ptail = threadIdx.x < 256 && pb < p.B;
    float c0v = 0.f;
    LstmLive lv{true, 0.f};
    if (threadIdx.x < 256) {                                     // wave-uniform
        const int qb = min(pb, p.B - 1);
        c0v = p.pw.c0[qb * H + pj];
        lv = lstm_live_load(p.pw, qb, pj);
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < CPW; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    acc[t][q] = mfma16(comp(fa[i][t], c), comp(fb[i][q], c), acc[t][q]);

    if (threadIdx.x >= 256) {
        float* sp = &s_pre[r_gate][r_row * 8 + r_half * 4];
        sp[0] = pre4.x; sp[1] = pre4.y; sp[2] = pre4.z; sp[3] = pre4.w;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_red[wave][t * 2 + q][(kk * 4 + r) * 16 + li] = acc[t][q][r];
    __syncthreads();

    if (!ptail) return;
    float g4[4];
    const int tt = prow >> 4, rr = prow & 15;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v = s_pre[g][e4];
        const int e = rr * 16 + (g & 1) * 8 + pcol;
#pragma unroll
        for (int k = 0; k < LSTMR_WAVES; ++k) v += s_red[k][tt * 2 + (g >> 1)][e];
        g4[g] = v;
    }
    lstm_cell_update(p.pw, pb, pj, g4, c0v, lv);
}

// Fused BACKWARD time step of the encoder LSTM: block = 16 rows x 16 hidden units, 8 waves = 8
// K-slices of dh_{t+1}[tile] = dgates_{t+1}[16 rows, 4H] . W_hh^T[16 units, 4H] (all loads up front,
// partial tiles meet in LDS), then the cell backward of step t for the tile's 256 elements in the
// same launch: one dependent launch per time step instead of two.  grid (H/16, ceil(B/16)).
constexpr int BWS_WAVES = 8;

template <int CPW>
__global__ __launch_bounds__(BWS_WAVES * 64) void lstm_bwd_step_fused_kernel(LstmBwdStepArgs p) {
    __shared__ float s_part[BWS_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int H = p.H, B = p.B;
    const int j0 = blockIdx.x * 16, m0 = blockIdx.y * 16;

    // operands of the cell backward, fetched with the fragments (threads 0..255 own one element)
    const int prow = threadIdx.x >> 4, pcol = threadIdx.x & 15;
    const int pb = m0 + prow, pj = j0 + pcol;
    const bool ptail = threadIdx.x < 256 && pb < B;
    const int qb = min(pb, B - 1);
    const size_t idx = (size_t)qb * H + pj;
    const float* gp = p.gates + (size_t)qb * 4 * H + pj;
    const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
    const float c1 = p.c1[idx], c0 = p.c0[idx];
    const float dc = p.dc_in[idx];
    float dh = p.dh_in[idx];
    const bool dead = p.t >= p.lengths[qb];
    if (p.dctx) {                                                // block-uniform
        float v = p.dctx[((size_t)qb * p.T + p.t) * H + pj];
        if (p.ctx_drop.on()) {
            const uint32_t rk = drop_key(p.ctx_drop, (uint32_t)(p.ctx_drop.row0 + qb));
            v = dropout_keep(rk, (uint32_t)(p.t * H + pj), p.ctx_drop.thresh) ? v * p.ctx_drop.scale : 0.f;
        }
        dh += dead ? 0.f : v;                                    // (ctx beyond a row's length is the constant 0)
    }

    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    if (p.dgates_next) {                                         // block-uniform (absent at t = T-1)
        Seg2 sg;
        sg.s0 = Seg{p.dgates_next, 4 * H, p.w_hh_t, 4 * H, 4 * H};
        sg.n0 = (4 * H) >> 4;
        sg.s1 = sg.s0;
        sg.total = sg.n0;
        const int n = j0 + li;
        int mrow[1] = {min(m0 + li, B - 1)};
        const int c_lo = (wave * sg.total) / BWS_WAVES, c_hi = ((wave + 1) * sg.total) / BWS_WAVES;
        if (c_hi > c_lo) {
            Frags<1, CPW> f;
            upfront_load<1, CPW>(f, sg, c_lo, c_hi, n, mrow, kk);
            upfront_mma<1, CPW>(f, c_hi - c_lo, acc);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) s_part[wave][(kk * 4 + r) * 16 + li] = acc[0][r];
    __syncthreads();
    if (!ptail) return;
#pragma unroll
    for (int w = 0; w < BWS_WAVES; ++w) dh += s_part[w][threadIdx.x];

    float* dg = p.dgates + (size_t)pb * 4 * H + pj;
    const float tc = tanhf(c1);
    const float dout = dh * tc;
    const float dcl = dc + dh * og * (1.f - tc * tc);
    // packed sequence: a step that did not happen passes dh / dc through, dgates = 0
    dg[0] = dead ? 0.f : dcl * gg * ig * (1.f - ig);
    dg[H] = dead ? 0.f : dcl * c0 * fg * (1.f - fg);
    dg[2 * H] = dead ? 0.f : dcl * ig * (1.f - gg * gg);
    dg[3 * H] = dead ? 0.f : dout * og * (1.f - og);
    p.dc_out[(size_t)pb * H + pj] = dead ? dc : dcl * fg;
    p.dh_out[(size_t)pb * H + pj] = dead ? dh : 0.f;
}

// ------------------------------------------------------------------------------------------------
// NN: C[M,N] = A[M,K] * W[K,N]     (dX = dY * W; A K-contiguous, W N-contiguous)
// grid (ceil(N/256), ksplit, mblocks); wave = MT m-tiles x 64 columns (4 virtual tiles).
// ------------------------------------------------------------------------------------------------
struct NnArgs {
    const float* A;
    int lda;
    const float* W;
    int ldw;
    int M, N, K;
    int ksplit;
    float* out;      // slabs [ksplit][M][N] or final
    int ldo;
    int accumulate;  // direct mode only
};

template <int MT>
__global__ __launch_bounds__(256) void gemm_nn_kernel(NnArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * 64;
    if (n0 >= a.N) return;
    const int split = blockIdx.y;
    const int m0 = blockIdx.z * (16 * MT);
    const int li = lane & 15, kk = lane >> 4;
    const int ncol = n0 + 4 * li;                 // this lane's 4 consecutive columns
    const bool colok = ncol < a.N;                // N % 4 == 0
    const int ncl = colok ? ncol : 0;

    int mrow[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) mrow[t] = min(m0 + 16 * t + li, a.M - 1);

    f32x4 acc[MT][4];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[t][v] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int chunks = (a.K + 15) >> 4;
    const int c0 = (int)(((long)split * chunks) / a.ksplit);
    const int c1 = (int)(((long)(split + 1) * chunks) / a.ksplit);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int ch = c0; ch < c1; ++ch) {
        const int k = ch * 16 + 4 * kk;           // this lane's 4 consecutive k
        float4 bw[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            bw[c] = (k + c < a.K) ? ld4(a.W + (size_t)(k + c) * a.ldw + ncl) : z;
        float4 av[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) av[t] = (k < a.K) ? ld4(a.A + (size_t)mrow[t] * a.lda + k) : z;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int t = 0; t < MT; ++t)
                    acc[t][v] = mfma16(comp(av[t], c), comp(bw[c], v), acc[t][v]);
    }

    if (!colok) return;
    float* out = a.out + (a.ksplit > 1 ? (size_t)split * a.M * a.N : 0);
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + 16 * t + kk * 4 + r;
            if (row >= a.M) continue;
            float4 v = make_float4(acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]);
            float4* p = reinterpret_cast<float4*>(out + (size_t)row * a.ldo + ncol);
            if (a.ksplit == 1 && a.accumulate) {
                const float4 o = *p;
                v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
            }
            *p = v;
        }
}

// ------------------------------------------------------------------------------------------------
// TN: out[P,Q] (+)= Y[M,P]^T * X[M,Q]   (weight gradients; reduction over the batch rows)
// grid (ceil(Q/256), ceil(P/64)); wave = 64 P-rows x 64 Q-cols (4 x 4 virtual tiles).
// ------------------------------------------------------------------------------------------------
struct TnArgs {
    const float* Y;
    int ldy;
    const float* X;
    int ldx;
    int M, P, Q;
    float* out;
    int ldo;
    int accumulate;
    int msplit;            // > 1: block z reduces rows [z*M/msplit, (z+1)*M/msplit) into slab z of `out`
};

__global__ __launch_bounds__(256) void gemm_tn_kernel(TnArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int q0 = (blockIdx.x * 4 + wave) * 64;
    if (q0 >= a.Q) return;
    const int p0 = blockIdx.y * 64;
    if (a.msplit > 1) {    // row range of this split; its slab is a dense [P, Q] matrix
        const int z = blockIdx.z;
        const int m_lo = (int)(((long)z * a.M) / a.msplit), m_hi = (int)(((long)(z + 1) * a.M) / a.msplit);
        a.Y += (size_t)m_lo * a.ldy;
        a.X += (size_t)m_lo * a.ldx;
        a.M = m_hi - m_lo;
        a.out += (size_t)z * a.P * a.ldo;
    }
    const int li = lane & 15, kk = lane >> 4;
    const int pc = p0 + 4 * li;                 // Y columns pc..pc+3 (must be readable: ldy padded)
    const int qc = q0 + 4 * li;
    const bool pok = pc < a.ldy;                // stay inside the row (caller pads P to %4 via ldy)
    const bool qok = qc < a.Q;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // 8-deep clamped prefetch ring over the batch rows (4 rows per step): loads of steps s+1..s+7
    // are in flight while step s feeds 16 MFMAs; clamped (not predicated) addresses keep the loop
    // body branch-free, rows >= M contribute through a zero multiplier.
    const int steps = (a.M + 3) >> 2;
    const int pcl = pok ? pc : 0, qcl = qok ? qc : 0;
    auto ld = [&](int s, float4& yv, float4& xv) {
        const int m = min(4 * min(s, steps - 1) + kk, a.M - 1);
        yv = ld4(a.Y + (size_t)m * a.ldy + pcl);
        xv = ld4(a.X + (size_t)m * a.ldx + qcl);
    };
    auto mma = [&](int s, const float4& yv, const float4& xv) {
        const float z = (4 * s + kk < a.M && pok) ? 1.f : 0.f;     // tail rows / columns beyond P
        const float4 y = make_float4(yv.x * z, yv.y * z, yv.z * z, yv.w * z);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(comp(y, i), comp(xv, j), acc[i][j]);
    };
    constexpr int RING = 8;
    float4 yr[RING], xr[RING];
#pragma unroll
    for (int i = 0; i < RING; ++i) ld(i, yr[i], xr[i]);
    int s4 = 0;
    for (; s4 + RING <= steps; s4 += RING) {
#pragma unroll
        for (int i = 0; i < RING; ++i) {
            mma(s4 + i, yr[i], xr[i]);
            ld(s4 + RING + i, yr[i], xr[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < RING - 1; ++i)
        if (s4 + i < steps) mma(s4 + i, yr[i], xr[i]);

    if (!qok) return;
    // read-modify-write of the gradient tile: all 16 reads first (straight-line, clamped rows), then
    // the adds and stores -- one memory round trip instead of sixteen
    float4 w[4][4];
    if (a.accumulate) {                                  // block-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = min(p0 + 4 * (kk * 4 + r) + i, a.P - 1);
                w[i][r] = ld4(a.out + (size_t)p * a.ldo + qc);
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = p0 + 4 * (kk * 4 + r) + i;     // tile row (kk*4+r) is virtual: stride-4 rows
            float4 v = make_float4(acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]);
            if (a.accumulate) {
                v.x += w[i][r].x; v.y += w[i][r].y; v.z += w[i][r].z; v.w += w[i][r].w;
            }
            if (p < a.P) *reinterpret_cast<float4*>(a.out + (size_t)p * a.ldo + qc) = v;
        }
}

// ------------------------------------------------------------------------------------------------
// split-K reduce + epilogue
// ------------------------------------------------------------------------------------------------
struct RedArgs {
    const float* slabs;
    int ks;
    int M, N;
    float* y;
    int ldy;
    const float* bias;
    const float* bias2;
    const float* mul;
    float* y_pre;
    int ldy_pre;
    int epi;
    int accumulate;
};

__global__ __launch_bounds__(256) void reduce_slabs_kernel(RedArgs a) {
    const size_t total = (size_t)a.M * a.N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / a.N), col = (int)(i % a.N);
        float v = 0.f;
        for (int s = 0; s < a.ks; ++s) v += a.slabs[(size_t)s * total + i];
        if (a.bias) v += a.bias[col];
        if (a.bias2) v += a.bias2[col];
        if (a.epi == EPI_TANH) v = tanhf(v);
        if (a.epi == EPI_MUL) {
            if (a.y_pre) a.y_pre[(size_t)row * a.ldy_pre + col] = v;
            v *= a.mul[col];
        }
        float* o = a.y + (size_t)row * a.ldy + col;
        *o = a.accumulate ? *o + v : v;
    }
}

// out[n] (+)= sum_m Y[m,n]: block = 64 columns x 16 row groups, coalesced 256-B row segments.
// grid (ceil(N/64), msplit): with msplit > 1 block (x, z) sums rows [z*M/msplit, ...) into
// part[z][n] and a second tiny launch adds the parts (deterministic).  out2 (optional) receives
// the same sums (LSTM: b_ih and b_hh have the same gradient).
__global__ __launch_bounds__(1024) void colsum_kernel(const float* Y, int ldy, int M, int N,
                                                      float* out, float* out2, int accumulate,
                                                      int msplit, float* part) {
    __shared__ float s_p[16][64];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int z = blockIdx.y;
    const int m_lo = (int)(((long)z * M) / msplit), m_hi = (int)(((long)(z + 1) * M) / msplit);
    const int nc = min(n, N - 1);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;      // 4 independent loads in flight per thread
    int m = m_lo + g;
    for (; m + 48 < m_hi; m += 64) {
        s0 += Y[(size_t)m * ldy + nc];
        s1 += Y[(size_t)(m + 16) * ldy + nc];
        s2 += Y[(size_t)(m + 32) * ldy + nc];
        s3 += Y[(size_t)(m + 48) * ldy + nc];
    }
    for (; m < m_hi; m += 16) s0 += Y[(size_t)m * ldy + nc];
    s_p[g][c] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (g == 0 && n < N) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += s_p[k][c];
        if (msplit > 1) {
            part[(size_t)z * N + n] = t;
        } else {
            out[n] = accumulate ? out[n] + t : t;
            if (out2) out2[n] = accumulate ? out2[n] + t : t;
        }
    }
}

__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* part, int msplit, int N,
                                                            float* out, float* out2, int accumulate) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float t = 0.f;
    for (int z = 0; z < msplit; ++z) t += part[(size_t)z * N + n];
    out[n] = accumulate ? out[n] + t : t;
    if (out2) out2[n] = accumulate ? out2[n] + t : t;
}

// The same product with the operands shared through LDS: block = 4 waves = 2 x 2 tiles of 64 x 64,
// i.e. 128 P-rows x 128 Q-cols; every 16 batch rows are staged once ([16][128] of Y and of X, 16 KB,
// double buffered) and read back as fragments by the two waves that need them.  The register-
// streaming kernel above pulls 2 KB per wave and 16 MFMAs -- at the matrix-pipe rate that is the
// ~40 GB/s one CU sustains; this one pulls half of that.  A fragment row is 256 contiguous bytes
// per 16 lanes: conflict-free without padding.
constexpr int TNT_BM = 16;             // (TNT_B = 128: sf_gemm_plan.h)

__global__ __launch_bounds__(256) void gemm_tn_tiled_kernel(TnArgs a) {
    __shared__ float4 Ys[2][TNT_BM][TNT_B / 4];
    __shared__ float4 Xs[2][TNT_BM][TNT_B / 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp = wave >> 1, wq = wave & 1;
    const int p0b = blockIdx.y * TNT_B, q0b = blockIdx.x * TNT_B;
    if (a.msplit > 1) {    // row range of this split; its slab is a dense [P, Q] matrix
        const int z = blockIdx.z;
        const int m_lo = (int)(((long)z * a.M) / a.msplit), m_hi = (int)(((long)(z + 1) * a.M) / a.msplit);
        a.Y += (size_t)m_lo * a.ldy;
        a.X += (size_t)m_lo * a.ldx;
        a.M = m_hi - m_lo;
        a.out += (size_t)z * a.P * a.ldo;
    }
    const int li = lane & 15, kk = lane >> 4;
    const int srow = tid >> 5, sc4 = tid & 31;          // staging: 8 rows x 32 float4 per pass, 2 passes
    const int pcl = min(p0b + 4 * sc4, a.ldy - 4);      // clamped: columns beyond P / Q are never stored
    const int qcl = min(q0b + 4 * sc4, a.Q - 4);
    const int stages = (a.M + TNT_BM - 1) / TNT_BM;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 ry[2], rx[2];
    auto gload = [&](int st) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = min(st * TNT_BM + srow + 8 * h, a.M - 1);
            ry[h] = ld4(a.Y + (size_t)m * a.ldy + pcl);
            rx[h] = ld4(a.X + (size_t)m * a.ldx + qcl);
        }
    };
    auto lstore = [&](int st, int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool ok = st * TNT_BM + srow + 8 * h < a.M;    // rows beyond M contribute zeros
            Ys[buf][srow + 8 * h][sc4] = ok ? ry[h] : make_float4(0.f, 0.f, 0.f, 0.f);
            Xs[buf][srow + 8 * h][sc4] = rx[h];
        }
    };
    gload(0);
    lstore(0, 0);
    __syncthreads();
    for (int st = 0; st < stages; ++st) {
        const int buf = st & 1;
        gload(min(st + 1, stages - 1));                          // clamped, not predicated
#pragma unroll
        for (int s = 0; s < TNT_BM / 4; ++s) {
            const float4 y = Ys[buf][4 * s + kk][wp * 16 + li];
            const float4 x = Xs[buf][4 * s + kk][wq * 16 + li];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(comp(y, i), comp(x, j), acc[i][j]);
        }
        lstore(st + 1, buf ^ 1);                                 // (st + 1 == stages: all rows >= M -> zeros)
        __syncthreads();
    }

    const int p0 = p0b + wp * 64, qc = q0b + wq * 64 + 4 * li;
    if (qc >= a.Q) return;
    float4 w[4][4];
    if (a.accumulate) {                                  // block-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = min(p0 + 4 * (kk * 4 + r) + i, a.P - 1);
                w[i][r] = ld4(a.out + (size_t)p * a.ldo + qc);
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = p0 + 4 * (kk * 4 + r) + i;     // tile row (kk*4+r) is virtual: stride-4 rows
            float4 v = make_float4(acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]);
            if (a.accumulate) {
                v.x += w[i][r].x; v.y += w[i][r].y; v.z += w[i][r].z; v.w += w[i][r].w;
            }
            if (p < a.P) *reinterpret_cast<float4*>(a.out + (size_t)p * a.ldo + qc) = v;
        }
}

// ------------------------------------------------------------------------------------------------
// TN on the bf16 matrix cores (round 4): the weight gradients out[P,Q] (+)= Y[M,P]^T X[M,Q] as bf16x6 split products
// (sf_split.h: fp32-class accuracy, 6/16 of the fp32-MFMA time).  v_mfma_f32_16x16x32_bf16 wants, per lane, EIGHT
// consecutive values of the reduction index for one output row / column -- here eight different batch rows m of one
// column of Y (or X): the operands are transposed on their way into LDS.
//   block = 4 waves = 2 x 2 wave tiles of 64 x 64 -> 128 P-rows x 128 Q-cols; a stage = 64 batch rows.
//   staging: a thread loads an 8 (m) x 4 (columns) patch of Y and of X (8 + 8 float4), splits each COLUMN's eight values
//   into three bf16x8 pieces and stores each as one ds_write_b128 into plane[piece][column][m]: LDS rows = tile columns,
//   64 m = 128 bytes, 16-byte chunks XOR-swizzled with (row >> 1) -- the lanes of every write and of every fragment
//   read spread evenly over the eight chunk positions.  One stage buffer (96 KB: 2 operands x 3 planes x 16 KB, one
//   workgroup per CU); the next stage's global loads are in flight in registers while the 192 MFMAs of a stage run.
//   MEASURED (round 4): 3.8 us per stage where the MFMAs alone take 1.3 -- the split costs ~8 VALU operations per value
//   and every element of Y is split again by each of the Q / 128 column blocks; with one wave per SIMD the split, the
//   LDS traffic and the matrix pipe take turns.  It wins where the reduction is deep and the output small (the
//   encoder's dW_hh over T*B = 8 000 rows: 196 -> 131 us) and loses on the decoder's dW_ih (320 -> 351 us), so the
//   dispatch uses it for M >= 4096 only.  A variant that splits stage s+1 column by column between the MFMA groups
//   of stage s (32-row stages, two LDS buffers, one barrier per stage) was built and is slower still (210 us on the
//   encoder shape: 256 AGPRs, twice the barriers).  The next step is operands split ONCE (a pre-pass writing bf16
//   planes [column][m]) so that the product kernel only copies.
//   split-M over grid.z into slabs for small outputs (same reduce_slabs as the fp32 kernels: deterministic order).
// ------------------------------------------------------------------------------------------------
constexpr int TNS_K = 64, TNS_ROWB = 128;             // (TNS_B = 128: sf_gemm_plan.h)
constexpr int TNS_PLANE = TNS_B * TNS_ROWB;           // one piece plane of one operand: 16 KB
static_assert(TNS_LDS == 2 * 3 * TNS_PLANE, "sf_gemm_plan.h: the stage buffer of gemm_tn_split_kernel");

__global__ __launch_bounds__(256, 1) void gemm_tn_split_kernel(TnArgs a) {
    extern __shared__ __align__(16) unsigned char tns_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp = wave >> 1, wq = wave & 1;
    const int p0b = blockIdx.y * TNS_B, q0b = blockIdx.x * TNS_B;
    if (a.msplit > 1) {    // row range of this split; its slab is a dense [P, Q] matrix
        const int z = blockIdx.z;
        const int m_lo = (int)(((long)z * a.M) / a.msplit), m_hi = (int)(((long)(z + 1) * a.M) / a.msplit);
        a.Y += (size_t)m_lo * a.ldy;
        a.X += (size_t)m_lo * a.ldx;
        a.M = m_hi - m_lo;
        a.out += (size_t)z * a.P * a.ldo;
    }
    const int mg = lane >> 3, cg = wave * 8 + (lane & 7);       // staging patch: rows 8 mg .. +7 of the stage, columns 4 cg .. +3
    const int li = lane & 15, kk = lane >> 4;
    const int stages = (a.M + TNS_K - 1) / TNS_K;
    const float* yp = a.Y + p0b + 4 * cg;
    const float* xp = a.X + q0b + 4 * cg;

    f32x4 hi[4][4], lo[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) hi[i][j] = lo[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 ry[8], rx[8];
    auto gload = [&](int st) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int m = min(st * TNS_K + 8 * mg + r, a.M - 1);  // clamped, not predicated
            ry[r] = ld4(yp + (size_t)m * a.ldy);
            rx[r] = ld4(xp + (size_t)m * a.ldx);
        }
    };
    auto lstore = [&](int st) {
        const int live = a.M - (st * TNS_K + 8 * mg);             // rows of this patch inside the batch
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float z = r < live ? 1.f : 0.f;                 // rows beyond M contribute zeros
            ry[r] = make_float4(ry[r].x * z, ry[r].y * z, ry[r].z * z, ry[r].w * z);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int row = 4 * cg + c;
            const int off = row * TNS_ROWB + ((mg ^ (row >> 1)) & 7) * 16;
            const Split8 sy = split3_f8(make_float4(comp(ry[0], c), comp(ry[1], c), comp(ry[2], c), comp(ry[3], c)),
                                        make_float4(comp(ry[4], c), comp(ry[5], c), comp(ry[6], c), comp(ry[7], c)));
            const Split8 sx = split3_f8(make_float4(comp(rx[0], c), comp(rx[1], c), comp(rx[2], c), comp(rx[3], c)),
                                        make_float4(comp(rx[4], c), comp(rx[5], c), comp(rx[6], c), comp(rx[7], c)));
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                *reinterpret_cast<bf16x8*>(tns_smem + pl * TNS_PLANE + off) = sy.p[pl];
                *reinterpret_cast<bf16x8*>(tns_smem + (3 + pl) * TNS_PLANE + off) = sx.p[pl];
            }
        }
    };

    gload(0);
    for (int st = 0; st < stages; ++st) {
        lstore(st);
        __syncthreads();
        gload(min(st + 1, stages - 1));                           // in flight while this stage's MFMAs run
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            Split8 fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rowa = wp * 64 + 16 * i + li, rowb = wq * 64 + 16 * i + li;
                const int offa = rowa * TNS_ROWB + (((4 * ks + kk) ^ (rowa >> 1)) & 7) * 16;
                const int offb = rowb * TNS_ROWB + (((4 * ks + kk) ^ (rowb >> 1)) & 7) * 16;
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    fa[i].p[pl] = *reinterpret_cast<const bf16x8*>(tns_smem + pl * TNS_PLANE + offa);
                    fb[i].p[pl] = *reinterpret_cast<const bf16x8*>(tns_smem + (3 + pl) * TNS_PLANE + offb);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) mfma_split6(fa[i], fb[j], hi[i][j], lo[i][j]);
        }
        __syncthreads();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // (the clamped prefetch of the last stage)

    // D[row 4 kk + r][col li] of every 16 x 16 tile; a gradient tile is read-modified-written 16 values at a time
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* orow = a.out + (size_t)(p0b + wp * 64 + 16 * i + 4 * kk) * a.ldo + q0b + wq * 64 + li;
        float old[4][4];
        if (a.accumulate) {                                       // block-uniform
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) old[j][r] = orow[(size_t)r * a.ldo + 16 * j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = hi[i][j][r] + lo[i][j][r];
                if (a.accumulate) v += old[j][r];
                orow[(size_t)r * a.ldo + 16 * j] = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// ISSUE.  Every entry below checks its arguments, asks sf_gemm_plan.h for a plan (which kernel, grid, splits, workspace
// layout: pure host code, tests/test_gemm_plan_host.py), fills the kernel's argument struct from the plan and the
// pointers, and launches.  Nothing here decides.
// ------------------------------------------------------------------------------------------------
static_assert((int)PLAN_OK == (int)SF_OK && (int)PLAN_UNSUPPORTED == (int)SF_ERR_UNSUPPORTED &&
              (int)PLAN_WORKSPACE == (int)SF_ERR_WORKSPACE, "sf_gemm_plan.h: PlanStatus");

inline GemmSwitches switches() {
    return GemmSwitches{g_nt_force_f32, g_nt_big, g_nt_big_ksplit, g_tn_split_min_rows, g_tn_group};
}
inline dim3 dim(const PlanGrid& g) { return dim3(g.x, g.y, g.z); }

// (with_index / SF_LAUNCH_INST, where a planned SMALL_INST, 1 .. NT_MT_MAX or NN_INST becomes a template argument: sf_common.h)
// A launch of a kernel that takes more than 64 KB of dynamic LDS: that must be opted into, once per instantiation
template <auto Kernel, class... Args>
void launch_big_lds(const char* name, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
    static const hipError_t opted = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)opted;
    SF_LAUNCH_AS(name, Kernel, grid, block, lds, st, args...);
}

// y (+)= epi(sum of the `ks` slabs [M][N] + bias), in a fixed order: deterministic
void reduce_slabs(const float* slabs, int ks, int M, int N, const LinearOut& o, hipStream_t st) {
    const RedArgs r{slabs, ks, M, N, o.y, o.ldy, o.bias, o.bias2, o.mul, o.y_pre, o.ldy_pre, o.epi, o.accumulate};
    SF_LAUNCH(reduce_slabs_kernel, dim3((int)std::min<size_t>(((size_t)M * N + 255) / 256, 2048)), dim3(256), 0, st, r);
}
inline LinearOut plain_out(float* y, int ldy, int accumulate) {
    LinearOut o{};
    o.y = y; o.ldy = ldy; o.epi = EPI_NONE; o.accumulate = accumulate;
    return o;
}

int nt_big_launch(const NtBigArgs& b, const PlanGrid& grid, hipStream_t st) {
    launch_big_lds<gemm_nt_big_kernel>("gemm_nt_big_kernel", dim(grid), dim3(512), (size_t)2 * 6 * NB_PLANE, st, b);
    return launch_status();
}

SmallArgs small_args(const Seg* segs, int nseg, int M, int N, const LinearOut& out) {
    SmallArgs sa{};
    sa.sg.s0 = segs[0];
    sa.sg.n0 = ceil_div(segs[0].K, 16);
    sa.sg.s1 = nseg == 2 ? segs[1] : segs[0];
    sa.sg.total = sa.sg.n0 + (nseg == 2 ? ceil_div(segs[1].K, 16) : 0);
    sa.M = M; sa.N = N; sa.y = out.y; sa.ldy = out.ldy; sa.bias = out.bias; sa.bias2 = out.bias2;
    sa.epi = out.epi; sa.mul = out.mul; sa.y_pre = out.y_pre; sa.ldy_pre = out.ldy_pre;
    sa.accumulate = out.accumulate;
    sa.aux = out.aux; sa.ld_aux = out.ld_aux; sa.addend = out.addend; sa.ld_addend = out.ld_addend;
    sa.r1_s = out.r1_s; sa.r1_v = out.r1_v;
    return sa;
}

}  // namespace

bool linear_small_plan(const Seg* segs, int nseg, int M, int N, const LinearOut& out,
                       SmallPlan* plan) {
    if (nseg < 1 || nseg > 2) return false;
    int chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        if (segs[s].K <= 0 || segs[s].K % 4 || segs[s].lda % 4 || segs[s].ldw % 4) return false;
        chunks += ceil_div(segs[s].K, 16);
    }
    if (!plan_detail::small_shape(M, N, chunks, &plan->mt, &plan->cpw)) return false;
    plan->args = small_args(segs, nseg, M, N, out);
    plan->gx = ceil_div(N, 16);
    plan->gy = ceil_div(ceil_div(M, 16), plan->mt);
    return true;
}

int launch_small_plan(const SmallPlan& p, hipStream_t st) {
    const SmallArgs& a = p.args;
    const bool extras = a.addend || a.r1_s || a.epi == EPI_TANHBWD;
    const dim3 grid(p.gx, p.gy), block(SMALL_WAVES * 64);
    const bool known = with_index<SMALL_INSTS>(small_inst(p.mt, p.cpw), [&](auto i) {
        constexpr int MT = SMALL_INST[decltype(i)::value].mt, CPW = SMALL_INST[decltype(i)::value].cpw;
        if (extras) SF_LAUNCH_INST(gemm_nt_small_x_kernel, (MT, CPW), grid, block, 0, st, a);
        else SF_LAUNCH_INST(gemm_nt_small_kernel, (MT, CPW), grid, block, 0, st, a);
    });
    return known ? launch_status() : SF_ERR_UNSUPPORTED;
}

size_t pack_bf16_bytes(int rows, int K) {
    if (rows <= 0 || K <= 0 || K % TBK) return 0;
    return (size_t)ceil_div(rows, 16) * (K / TBK) * BW_STAGE_BYTES;
}

int pack_bf16(const float* w, int ld, int rows, int K, void* out, hipStream_t st) {
    const size_t bytes = pack_bf16_bytes(rows, K);
    SF_CHECK_ARG(w && out && bytes && bytes / 16 < (1ull << 32) && ld >= K && ld % 4 == 0 &&
                 ((uintptr_t)w | (uintptr_t)out) % 16 == 0);
    const unsigned total = (unsigned)(bytes / 16);
    SF_LAUNCH(pack_bf16_kernel, dim3((total + 255) / 256), dim3(256), 0, st, w, ld, rows, K, (uint4*)out, total);
    return launch_status();
}

int linear_nt(const Seg* segs, int nseg, int M, int N, const LinearOut& out, float* ws,
              size_t ws_floats, hipStream_t st, float** raw_slabs, int* ksplit_out, const void* const* packed_w) {
    SF_CHECK_ARG(nseg >= 1 && nseg <= 3 && M > 0 && N > 0);
    NtAsk q{};
    for (int s = 0; s < nseg; ++s) {
        SF_CHECK_ARG(segs[s].K > 0 && segs[s].K % 4 == 0 && segs[s].lda % 4 == 0 &&
                     segs[s].ldw % 4 == 0);
        q.K[s] = segs[s].K;
    }
    q.M = M; q.N = N; q.nseg = nseg;
    q.raw_slabs = raw_slabs; q.ksplit_out = ksplit_out; q.packed_w = packed_w;
    q.epi = out.epi; q.accumulate = out.accumulate; q.addend = out.addend; q.r1_s = out.r1_s;
    q.ws_floats = ws ? ws_floats : 0;
    const NtPlan p = plan_nt(q, switches());
    if (p.status != PLAN_OK) return p.status;
    if (ksplit_out) *ksplit_out = p.ksplit;
    if (raw_slabs) *raw_slabs = ws;
    if (p.family == NT_SMALL)
        return launch_small_plan(SmallPlan{small_args(segs, nseg, M, N, out), p.mt, p.cpw, p.grid.x, p.grid.y}, st);
    if (p.family == NT_BIG) {
        NtBigArgs b{};
        for (int s = 0; s < nseg; ++s) b.seg[s] = segs[s];
        b.nseg = nseg; b.M = M; b.N = N; b.ksplit = p.ksplit;
        if (p.slabs) {                   // (raw slabs: the caller adds them up, and the bias, itself)
            b.y = ws; b.ldy = N; b.epi = EPI_NONE;
        } else {
            b.y = out.y; b.ldy = out.ldy; b.bias = out.bias; b.bias2 = out.bias2;
            b.addend = out.addend; b.ld_addend = out.ld_addend; b.epi = (int)out.epi; b.accumulate = out.accumulate;
        }
        return nt_big_launch(b, p.grid, st);
    }
    NtArgs a{};
    a.nseg = nseg;
    for (int s = 0; s < nseg; ++s) {
        a.seg[s] = segs[s];
        a.chunks_total += ceil_div(segs[s].K, 16);
    }
    a.M = M; a.N = N; a.ksplit = p.ksplit; a.epi = EPI_NONE;
    if (p.slabs) {
        a.out = ws; a.ldo = N;
    } else {                        // single split: bias and epilogue fused into the GEMM
        a.out = out.y; a.ldo = out.ldy; a.bias = out.bias; a.bias2 = out.bias2; a.epi = out.epi;
        a.accumulate = out.accumulate; a.mul = out.mul; a.y_pre = out.y_pre; a.ldy_pre = out.ldy_pre;
    }
    NtPackedW pk{};
    for (int s = 0; p.family == NT_BF16W && s < nseg; ++s) pk.p[s] = packed_w[s];
    const dim3 grid = dim(p.grid), block(p.block);
    const bool known = with_index<NT_MT_MAX>(p.mt - 1, [&](auto i) {
        constexpr int MT = decltype(i)::value + 1;
        switch (p.family) {
            case NT_BF16W:
                launch_big_lds<gemm_nt_bf16w_kernel<MT>>(inst_name<gemm_nt_bf16w_kernel<MT>, MT>("gemm_nt_bf16w_kernel"),
                                                         grid, block, p.lds, st, a, pk);
                break;
            case NT_SPLIT:
                launch_big_lds<gemm_nt_split_kernel<MT>>(inst_name<gemm_nt_split_kernel<MT>, MT>("gemm_nt_split_kernel"),
                                                         grid, block, p.lds, st, a);
                break;
            case NT_TILED:
                launch_big_lds<gemm_nt_tiled_kernel<MT>>(inst_name<gemm_nt_tiled_kernel<MT>, MT>("gemm_nt_tiled_kernel"),
                                                         grid, block, p.lds, st, a);
                break;
            default:
                SF_LAUNCH_INST(gemm_nt_kernel, (MT), grid, block, 0, st, a);
        }
    });
    if (!known) return SF_ERR_UNSUPPORTED;
    if (p.reduce) reduce_slabs(ws, p.ksplit, M, N, out, st);
    return launch_status();
}

int lstm_step_fused(const LstmStepArgs& p, hipStream_t st) {
    if (p.H % 16 || (p.x && (p.I % 4 || p.ldx % 4 || p.ld_w_ih % 4))) return SF_ERR_UNSUPPORTED;
    const int total = ceil_div(p.H, 16) + (p.x ? ceil_div(p.I, 16) : 0);
    // (p.wide: the decoder's step on gate-space rows takes them at every B -- its K = 640 needs lstm_step_fused_kernel<16>,
    //  which spills, 19.4 us at B = 16 -- profiles/gate_rows_attended_ab.txt)
    if ((p.B > 16 || p.wide) && p.H % 8 == 0) {          // 32 x 8 patches: fewer bytes per block (see the kernel)
        const int cw = ceil_div(total, LSTMW_WAVES);
        dim3 wgrid(p.H / 8, ceil_div(p.B, 32)), wblock(LSTMW_WAVES * 64);
        if (cw <= 2) {
            SF_LAUNCH(lstm_step_wide_kernel<2>, wgrid, wblock, 0, st, p);
            return launch_status();
        }
        if (cw <= 4) {
            SF_LAUNCH(lstm_step_wide_kernel<4>, wgrid, wblock, 0, st, p);
            return launch_status();
        }
    }
    const int c = ceil_div(total, LSTM_KS);
    dim3 grid(p.H / 16, ceil_div(p.B, 16)), block(4 * LSTM_KS * 64);
    if (c <= 8)
        SF_LAUNCH(lstm_step_fused_kernel<8>, grid, block, 0, st, p);
    else if (c <= 16)
        SF_LAUNCH(lstm_step_fused_kernel<16>, grid, block, 0, st, p);
    else
        return SF_ERR_UNSUPPORTED;
    return launch_status();
}

int lstm_step_rows(const LstmRowsArgs& p, hipStream_t st) {
    if (!recurrent_row_cell(p.K, p.H) || p.ldx % 4 || p.ldw % 4 || p.B < 1 || !p.x || !p.w || !p.xg_h || !p.xg || !p.xg2 ||
        (((uintptr_t)p.x | (uintptr_t)p.w | (uintptr_t)p.xg_h | (uintptr_t)p.xg | (uintptr_t)p.xg2) & 15))
        return SF_ERR_UNSUPPORTED;
    const dim3 grid(p.H / 8, ceil_div(p.B, 32)), block(LSTMR_WAVES * 64);
    if (ceil_div(ceil_div(p.K, 16), LSTMR_WAVES) <= 1)
        SF_LAUNCH(lstm_step_rows_kernel<1>, grid, block, 0, st, p);
    else
        SF_LAUNCH(lstm_step_rows_kernel<2>, grid, block, 0, st, p);
    return launch_status();
}

int lstm_bwd_step_fused(const LstmBwdStepArgs& p, hipStream_t st) {
    if (p.H % 16 || (4 * p.H) % 16) return SF_ERR_UNSUPPORTED;
    const int c = ceil_div((4 * p.H) >> 4, BWS_WAVES);
    dim3 grid(p.H / 16, ceil_div(p.B, 16)), block(BWS_WAVES * 64);
    if (c <= 8)
        SF_LAUNCH(lstm_bwd_step_fused_kernel<8>, grid, block, 0, st, p);
    else if (c <= 16)
        SF_LAUNCH(lstm_bwd_step_fused_kernel<16>, grid, block, 0, st, p);
    else
        return SF_ERR_UNSUPPORTED;
    return launch_status();
}

// NN split-K workspace is provided by a per-stream scratch owned by the API layer.
int gemm_nn_ws(const float* A, int lda, const float* W, int ldw, int M, int N, int K, float* y,
               int ldy, int accumulate, float* ws, size_t ws_floats, hipStream_t st) {
    SF_CHECK_ARG(M > 0 && N > 0 && K > 0 && N % 4 == 0 && lda % 4 == 0 && ldw % 4 == 0 &&
                 ldy % 4 == 0);
    const NnPlan p = plan_nn(M, N, K, ws ? ws_floats : 0);
    const bool slabs = p.ks > 1;
    const NnArgs a{A, lda, W, ldw, M, N, K, p.ks, slabs ? ws : y, slabs ? N : ldy, accumulate};
    const bool known = with_index<NN_INSTS>(nn_inst(p.mt), [&](auto i) {
        constexpr int MT = NN_INST[decltype(i)::value];
        SF_LAUNCH_INST(gemm_nn_kernel, (MT), dim(p.grid), dim3(256), 0, st, a);
    });
    if (!known) return SF_ERR_UNSUPPORTED;
    if (slabs) reduce_slabs(ws, p.ks, M, N, plain_out(y, ldy, accumulate), st);
    return launch_status();
}

int gemm_nn(const float* A, int lda, const float* W, int ldw, int M, int N, int K, float* y,
            int ldy, int accumulate, hipStream_t st) {
    return gemm_nn_ws(A, lda, W, ldw, M, N, K, y, ldy, accumulate, nullptr, 0, st);
}

namespace {

// The many-row form of a weight gradient (round 5): a SMALL weight matrix with a deep reduction (the eight [256..512] x
// [512..2176] weight gradients of the decoder over 2 000 stacked rows: 25 TFLOP/s in gemm_tn_kernel, 90 us each) as an NT
// product of the two TRANSPOSED operands on the LDS-tiled many-row kernel: dW[P,Q] += Y^T[P,M] (X^T[Q,M])^T (bf16x6, 3x
// closer to float64 than the fp32 kernels), into `ks` K-split slabs or, unsplit, straight into out.  gemm_tn and
// gemm_tn_group share it; they differ in the tile budget of plan_detail::many_row_ksplit and in who transposes.
NtBigArgs many_row_args(const TnJob& t, const float* yt, const float* xt, int ks, float* slabs) {
    NtBigArgs b{};
    b.seg[0] = Seg{yt, t.M, xt, t.M, t.M};
    b.nseg = 1; b.M = t.P; b.N = t.Q; b.epi = EPI_NONE; b.ksplit = ks;
    if (ks > 1) {
        b.y = slabs; b.ldy = t.Q;
    } else {
        b.y = t.out; b.ldy = t.ldo; b.accumulate = t.accumulate;
    }
    return b;
}

// A weight-gradient kernel into `splits` row slabs in the workspace and their sum, or straight into out
template <auto Kernel, bool BIG_LDS>
int tn_launch(const char* name, size_t lds, const TnJob& t, const TnPart& p, float* ws, hipStream_t st) {
    const bool slabs = p.splits > 1;
    const TnArgs a{t.Y, t.ldy, t.X, t.ldx, t.M, t.P, t.Q, slabs ? ws : t.out, slabs ? t.Q : t.ldo,
                   slabs ? 0 : t.accumulate, p.splits};
    if constexpr (BIG_LDS)
        launch_big_lds<Kernel>(name, dim(p.grid), dim3(256), lds, st, a);
    else
        SF_LAUNCH_AS(name, Kernel, dim(p.grid), dim3(256), lds, st, a);
    if (slabs) reduce_slabs(ws, p.splits, t.P, t.Q, plain_out(t.out, t.ldo, t.accumulate), st);
    return launch_status();
}

int tn_issue(const TnJob& t, const TnPart& p, float* ws, hipStream_t st) {
    switch (p.family) {
        case TN_MANY_ROW: {
            // two 32 x 32-tiled transposes into the workspace (~6 us each) + gemm_nt_big_kernel
            float* xt = ws + p.off_xt;
            float* slabs = ws + p.off_slabs;
            int rc = transpose_ld(t.Y, t.ldy, t.M, t.P, ws, st);
            if (rc != SF_OK) return rc;
            rc = transpose_ld(t.X, t.ldx, t.M, t.Q, xt, st);
            if (rc != SF_OK) return rc;
            rc = nt_big_launch(many_row_args(t, ws, xt, p.splits, slabs), p.grid, st);
            if (rc != SF_OK || p.splits == 1) return rc;
            reduce_slabs(slabs, p.splits, t.P, t.Q, plain_out(t.out, t.ldo, t.accumulate), st);
            return launch_status();
        }
        case TN_SPLIT: return tn_launch<gemm_tn_split_kernel, true>("gemm_tn_split_kernel", TNS_LDS, t, p, ws, st);
        case TN_TILED: return tn_launch<gemm_tn_tiled_kernel, false>("gemm_tn_tiled_kernel", 0, t, p, ws, st);
        case TN_STREAM: return tn_launch<gemm_tn_kernel, false>("gemm_tn_kernel", 0, t, p, ws, st);
        default: return SF_ERR_UNSUPPORTED;      // (a column cut is two parts: gemm_tn)
    }
}

}  // namespace

// Several weight gradients dW_j[P_j, Q_j] (+)= Y_j^T X_j over the same kind of stacked rows in THREE launches -- all the
// transposes (an operand two products share is transposed once), all the many-row products (gemm_nt_big_group_kernel),
// all the slab sums -- instead of four dependent launches per product.  Products outside the many-row form (or when
// the workspace is short) go through gemm_tn one by one.
int gemm_tn_group(const TnJob* jobs, int n, hipStream_t st, float* ws, size_t ws_floats) {
    for (int i = 0; i < n; ++i) {
        const TnJob& t = jobs[i];
        SF_CHECK_ARG(t.M > 0 && t.P > 0 && t.Q > 0 && t.Q % 4 == 0 && t.ldy % 4 == 0 && t.ldx % 4 == 0 && t.ldo % 4 == 0);
    }
    const TnGroupPlan g = plan_tn_group(jobs, n, ws ? ws_floats : 0, switches());
    if (g.grouped) {
        TrGroup tr{};
        NtBigGroup gg{};
        RedGroup rg{};
        for (int j = 0; j < g.ntr; ++j) {
            const TnJob& t = jobs[g.job[g.tr[j].job]];
            tr.p[j] = g.tr[j].x ? TrGroup::P{t.X, ws + g.tr[j].off, t.ldx, t.M, t.Q}
                                : TrGroup::P{t.Y, ws + g.tr[j].off, t.ldy, t.M, t.P};
            tr.first[j + 1] = tr.first[j] + ceil_div(tr.p[j].C, 32) * ceil_div(t.M, 32);
        }
        tr.n = g.ntr;
        for (int k = 0; k < g.n; ++k) {
            const TnJob& t = jobs[g.job[k]];
            float* slabs = ws + g.off_slabs[k];
            gg.job[k] = many_row_args(t, tr.p[g.yt[k]].dst, tr.p[g.xt[k]].dst, g.ks[k], slabs);
            gg.first[k + 1] = gg.first[k] + ceil_div(t.P, NB_T) * ceil_div(t.Q, NB_T) * g.ks[k];
            if (g.ks[k] > 1) rg.j[k] = RedGroup::J{slabs, t.out, g.ks[k], t.P, t.Q, t.ldo, t.accumulate};
        }
        gg.n = g.n;
        SF_LAUNCH(transpose_group_kernel, dim3(tr.first[tr.n]), dim3(256), 0, st, tr);
        launch_big_lds<gemm_nt_big_group_kernel>("gemm_nt_big_group_kernel", dim3(gg.first[g.n]), dim3(512),
                                                 (size_t)2 * 6 * NB_PLANE, st, gg);
        if (g.reduce)
            SF_LAUNCH(reduce_slabs_group_kernel, dim3((int)std::min<size_t>((g.most + 255) / 256, 2048), g.n), dim3(256), 0,
                      st, rg);
        const int rc = launch_status();
        if (rc != SF_OK) return rc;
    }
    for (int i = 0; i < n; ++i) {
        bool done = false;
        for (int k = 0; g.grouped && k < g.n; ++k) done = done || g.job[k] == i;
        if (done) continue;
        const TnJob& t = jobs[i];
        const int rc = gemm_tn(t.Y, t.ldy, t.X, t.ldx, t.M, t.P, t.Q, t.out, t.ldo, t.accumulate, st, ws, ws_floats);
        if (rc != SF_OK) return rc;
    }
    return SF_OK;
}

int gemm_tn(const float* Y, int ldy, const float* X, int ldx, int M, int P, int Q, float* out,
            int ldo, int accumulate, hipStream_t st, float* ws, size_t ws_floats) {
    SF_CHECK_ARG(M > 0 && P > 0 && Q > 0 && Q % 4 == 0 && ldy % 4 == 0 && ldx % 4 == 0 &&
                 ldo % 4 == 0);
    const TnJob t{Y, ldy, X, ldx, M, P, Q, out, ldo, accumulate};
    const TnPlan p = plan_tn(M, P, Q, ldy, ws ? ws_floats : 0, switches());
    if (p.family != TN_COLUMN_CUT) return tn_issue(t, p, ws, st);
    TnJob main = t, tail = t;
    main.Q = p.q_main;
    tail.X += p.q_main;
    tail.out += p.q_main;
    tail.Q = Q - p.q_main;
    const int rc = tn_issue(main, p.main, ws, st);
    return rc != SF_OK ? rc : tn_issue(tail, p.tail, ws, st);
}

int colsum(const float* Y, int ldy, int M, int N, float* out, int accumulate, hipStream_t st,
           float* out2, float* ws, size_t ws_floats) {
    SF_CHECK_ARG(M > 0 && N > 0);
    const ColsumPlan p = plan_colsum(M, N, ws ? ws_floats : 0);
    SF_LAUNCH(colsum_kernel, dim(p.grid), dim3(1024), 0, st, Y, ldy, M, N, out, out2, accumulate, p.ms, ws);
    if (p.ms > 1)
        SF_LAUNCH(colsum_finish_kernel, dim(p.finish), dim3(256), 0, st, ws, p.ms, N, out, out2, accumulate);
    return launch_status();
}

}  // namespace sf
