// The three soft attentions of the speaker/follower path, forward and backward.
// One workgroup per sample, row set resident in registers (see sf_rows.h).
#include <atomic>
#include "sf_kernels.h"
#include "sf_rows.h"
#include "sf_glue.h"
#include "sf_gemm_small.h"

namespace sf {

namespace {

// =================================================================================================
// Visual attention (model.py:310-326), V rows of F floats; CPL = 9 covers F <= 2304.
// MODE 0 (forward):  w_v = softmax_v(x_v . vec)             out = sum_v w_v x_v   (vec = q)
// MODE 1 (backward): d_v = x_v . vec, w_v = alpha_v (d_v - sum_u alpha_u d_u)      (vec = dout)
//                    out = dq = sum_v w_v x_v
// =================================================================================================
// (VIS_CPL, VIS_RPW, VIS_NW, VIS_SLOTS and every tile constant of this file that a dispatch rule reads: sf_attention_plan.h)

struct VisArgs {
    PanoSrc src;
    const float* vec;      // [B, ldvec]
    int ldvec;
    float* alpha;          // fwd: out [B,V]; bwd: in
    float* out;            // [B, ldo]
    int ldo;
    Dropout drop;          // fwd: applied to out; bwd: applied to vec (same mask)
    int drop_col0;
    const double* vec64;   // the query in float64 (visual_split_body<0, true>: scores accumulated in float64), or null
    int vec_slabs;         // MODE 1: `vec` is the sum of this many K-split slabs (0 / 1: a plain vector) ...
    long vec_slab_stride;  // ... `vec_slab_stride` floats apart: the workgroup adds them up itself (no reduce launch)
    // PROJ bodies only (visual_split_body<.., PROJ>): the scores come from PROJECTED rows -- `vec` is h1 [B, ldvec], not q
    const float* pv;       // [n_vp * V, ldp]: row n = [x_n^T M_v[:IMG, :] | x_n . c_v[:IMG]]
    const float* lv;       // [V * V, ldp]: the same of the location-embedding table's rows
    int ldp, pH;           // row stride of both (floats, a multiple of 4); H (the constant sits at column H)
    // proj_merge_body only: the first src.IMG floats of the merged sum go to out_img [B, ld_img] and `out` takes the
    // location part alone, from its column 0 (null: the whole sum to `out`)
    float* out_img;
    int ld_img;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, WAVE));
    return v;
}

template <int MODE, bool H16 = false>
__device__ __forceinline__ void visual_attn_body(const VisArgs& a, int b) {
    __shared__ float4 slots[VIS_SLOTS][VIS_CPL * 64];
    __shared__ float s_score[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int V = a.src.V;
    const int n4 = (a.src.IMG + a.src.LOC) >> 2;

    const PanoRow prow = pano_row<H16>(a.src, b);
    float4 x[VIS_RPW][VIS_CPL];
#pragma unroll
    for (int r = 0; r < VIS_RPW; ++r) {
        const int v = wave * VIS_RPW + r;
#pragma unroll
        for (int i = 0; i < VIS_CPL; ++i) {
            const int c = lane + 64 * i;
            x[r][i] = pano_load<H16>(prow, v, c, v < V && c < n4, V, n4);
        }
    }

    const uint32_t rkey = drop_key(a.drop, (uint32_t)(a.drop.row0 + b));
    float dot[VIS_RPW];
#pragma unroll
    for (int r = 0; r < VIS_RPW; ++r) dot[r] = 0.f;
    // (all chunks of the vector requested before the first use: behind the dropout branch below each load
    //  would otherwise be its own memory round trip)
    float4 qv[VIS_CPL];
    if (MODE == 1 && a.vec_slabs > 1) {
        // the vector arrives as K-split slabs of the product that formed it (the LSTM's data gradient): thread c adds
        // up float4 c of this row in slab order (the order reduce_slabs_kernel uses: same bits) into LDS, once per
        // workgroup, while the panorama rows are still on their way
        __shared__ float4 s_vec[VIS_CPL * 64];
        const int c = threadIdx.x;
        if (c < n4) {
            const float4* p0 = reinterpret_cast<const float4*>(a.vec + (size_t)b * a.ldvec) + c;
            float4 t = *p0;
            for (int sl = 1; sl < a.vec_slabs; ++sl) {
                const float4 u = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p0) + (size_t)sl * a.vec_slab_stride);
                t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
            }
            s_vec[c] = t;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VIS_CPL; ++i) qv[i] = s_vec[min(lane + 64 * i, n4 - 1)];
    } else {
#pragma unroll
    for (int i = 0; i < VIS_CPL; ++i)
        qv[i] = reinterpret_cast<const float4*>(a.vec + (size_t)b * a.ldvec)[min(lane + 64 * i, n4 - 1)];
    }
#pragma unroll
    for (int i = 0; i < VIS_CPL; ++i) {
        const int c = lane + 64 * i;
        float4 q = qv[i];
        if (c >= n4) q = f4zero();
        {
            if (MODE == 1 && a.drop.on()) {
                const uint32_t col = (uint32_t)(a.drop_col0 + 4 * c);
                q.x = dropout_keep(rkey, col + 0, a.drop.thresh) ? q.x * a.drop.scale : 0.f;
                q.y = dropout_keep(rkey, col + 1, a.drop.thresh) ? q.y * a.drop.scale : 0.f;
                q.z = dropout_keep(rkey, col + 2, a.drop.thresh) ? q.z * a.drop.scale : 0.f;
                q.w = dropout_keep(rkey, col + 3, a.drop.thresh) ? q.w * a.drop.scale : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < VIS_RPW; ++r) dot[r] += dot4(x[r][i], q);
    }
#pragma unroll
    for (int r = 0; r < VIS_RPW; ++r) {
        const float s = wave_sum(dot[r]);
        const int v = wave * VIS_RPW + r;
        if (lane == 0 && v < V) s_score[v] = s;
    }
    __syncthreads();

    // every wave redoes the V-wide softmax with lane v holding score v (V <= 64)
    const float s = lane < V ? s_score[lane] : -INFINITY;
    float w;
    if (MODE == 0) {
        const float m = wave_max(s);
        const float e = lane < V ? expf(s - m) : 0.f;
        w = e / wave_sum(e);
        if (wave == 0 && lane < V) a.alpha[(size_t)b * V + lane] = w;
    } else {
        const float alv = a.alpha[(size_t)b * V + min(lane, V - 1)];
        const float al = lane < V ? alv : 0.f;
        const float d = lane < V ? s : 0.f;
        w = al * (d - wave_sum(al * d));
    }

    float4 p[VIS_CPL];
#pragma unroll
    for (int i = 0; i < VIS_CPL; ++i) p[i] = f4zero();
#pragma unroll
    for (int r = 0; r < VIS_RPW; ++r) {
        const int v = wave * VIS_RPW + r;
        const float wr = __shfl(w, v < V ? v : 0, WAVE);
        if (v < V) {
#pragma unroll
            for (int i = 0; i < VIS_CPL; ++i) f4fma(p[i], wr, x[r][i]);
        }
    }

    float* orow = a.out + (size_t)b * a.ldo;
    const Dropout dr = a.drop;
    const int col0 = a.drop_col0;
    block_row_sum<VIS_CPL, VIS_NW, VIS_SLOTS>(p, slots, n4, [&](int c, float4 t) {
        if (MODE == 0 && dr.on()) {
            const uint32_t col = (uint32_t)(col0 + 4 * c);
            t.x = dropout_keep(rkey, col + 0, dr.thresh) ? t.x * dr.scale : 0.f;
            t.y = dropout_keep(rkey, col + 1, dr.thresh) ? t.y * dr.scale : 0.f;
            t.z = dropout_keep(rkey, col + 2, dr.thresh) ? t.z * dr.scale : 0.f;
            t.w = dropout_keep(rkey, col + 3, dr.thresh) ? t.w * dr.scale : 0.f;
        }
        reinterpret_cast<float4*>(orow)[c] = t;
    });
}

template <int MODE, bool H16 = false>
__global__ __launch_bounds__(VIS_NW * 64) void visual_attn_kernel(VisArgs a) {
    visual_attn_body<MODE, H16>(a, blockIdx.x);
}

// -------------------------------------------------------------------------------------------------
// Forward visual attention split over TWO workgroups per sample.  One workgroup per sample leaves
// 156 of 256 CUs idle at batch 100 and a CU sustains only ~20-35 GB/s of loads, so the 313 KB
// panorama of a sample took ~17 us to arrive; two half-panoramas on two CUs take half of that.
// Each block keeps flash-style partials of ITS 18 views (max m, sum l = sum e^(s-m), unnormalised
// weighted sum P, raw scores) in the workspace; the block that finishes second (ticket from a
// monotonic per-sample counter; partials are published write-through and read back with sc1
// loads, so no cache-wide fence is needed) merges: no spinning, no extra launch.
// -------------------------------------------------------------------------------------------------
struct VisSplit {
    float* part;          // [B][G][F + 64]: P | scores[32] | m, l
    unsigned* counter;    // [B] monotonic tickets (zero before the first launch)
    unsigned long long* trace;   // development aid (sf_debug_trace): [blocks][8] wall-clock stamps
};
__device__ __forceinline__ void vis_stamp(const VisSplit& sp, int block, int slot) {
    if (sp.trace && threadIdx.x == 0) sp.trace[(size_t)block * 8 + slot] = wall_clock64();
}

// PHASE 0: partials + ticket + merge by the last arriver, in one launch (hand-off inside the launch:
//          write-through stores, sc1 loads).
// PHASE 1: partials only, PHASE 2: merge only -- the same two halves as two consecutive launches
//          (plain stores / loads: the kernel boundary is the hand-off).  The pipelined decode step
//          runs them beside two different small products, so the visual attention of step t+1 never
//          holds up the text / scoring chain of step t.
// F64 (PHASE 0 only; the speaker's path encoder, csrc/sf_precise.hip): the query arrives in float64 and every score is
//          accumulated in float64; a group's record holds its scores RELATIVE to its own maximum (small numbers:
//          exact in fp32 to 1e-7 of the softmax weight, where a raw score of +-80 would carry 4e-6) and that maximum as a
//          float64 in two dwords.
// PROJ (the projected decode chain, sf_api_follower.hip: tail_proj): x_v . q with q = M_v h1 + c_v is re-associated to
//          (x_v^T M_v) . h1 + x_v . c_v, and the bracket is a row of a table built once per (feature table, weights):
//          score_v = (PV[row_v][:H] + LV[view * V + v][:H]) . h1 + PV[row_v][H] + LV[..][H].  The query q is never
//          formed; the rows themselves are still loaded (the weighted sum needs them) and the record is unchanged.
template <int PHASE, bool F64 = false, bool H16 = false, bool PROJ = false>
__device__ __forceinline__ void visual_split_body(const VisArgs& a, const VisSplit& sp, int g, int b) {
    __shared__ float4 slots[VSP_SLOTS][VIS_CPL * 64];
    __shared__ float s_score[64];
    __shared__ double s_score64[F64 ? 32 : 1];
    __shared__ int s_last;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.src.V;
    const int F = a.src.IMG + a.src.LOC, n4 = F >> 2;
    const int pstride = F + 64;
    float* rec = sp.part + ((size_t)b * VSP_G + g) * pstride;

    if (PHASE != 2) {
    vis_stamp(sp, b * VSP_G + g, 0);
    const PanoRow prow = pano_row<H16>(a.src, b);
    float4 x[VIS_RPW][VIS_CPL];
#pragma unroll
    for (int r = 0; r < VIS_RPW; ++r) {
        const int v = g * VSP_RPG + wave * VIS_RPW + r;
#pragma unroll
        for (int i = 0; i < VIS_CPL; ++i) {
            const int c = lane + 64 * i;
            x[r][i] = pano_load<H16>(prow, v, c, v < V && c < n4, V, n4);
        }
    }
    float s, m, e;          // F64: s = score - m (relative), m unused (md holds the maximum)
    double md = 0.0;
    if (F64) {
        double dot[VIS_RPW];
#pragma unroll
        for (int r = 0; r < VIS_RPW; ++r) dot[r] = 0.0;
        const double* qrow = a.vec64 + (size_t)b * a.ldvec;
#pragma unroll
        for (int i = 0; i < VIS_CPL; ++i) {
            const int c = lane + 64 * i, cc = min(c, n4 - 1);
            const double2 q0 = reinterpret_cast<const double2*>(qrow)[2 * cc], q1 = reinterpret_cast<const double2*>(qrow)[2 * cc + 1];
            const double k = c < n4 ? 1.0 : 0.0;
#pragma unroll
            for (int r = 0; r < VIS_RPW; ++r) {
                double t = (double)x[r][i].x * q0.x;
                t = fma((double)x[r][i].y, q0.y, t);
                t = fma((double)x[r][i].z, q1.x, t);
                t = fma((double)x[r][i].w, q1.y, t);
                dot[r] = fma(t, k, dot[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < VIS_RPW; ++r) {
            const double sd = wave_sum_f64(dot[r]);
            const int vl = wave * VIS_RPW + r;
            if (lane == 0) s_score64[vl] = (g * VSP_RPG + vl < V) ? sd : -INFINITY;
        }
        __syncthreads();
        vis_stamp(sp, b * VSP_G + g, 1);
        const double sd = lane < VSP_RPG ? s_score64[lane] : -INFINITY;
        md = wave_max_f64(sd);
        s = sd > -INFINITY ? (float)(sd - md) : -INFINITY;
        m = 0.f;
        e = sd > -INFINITY ? expf(s) : 0.f;
    } else {
    float dot[VIS_RPW], cadd[VIS_RPW];
#pragma unroll
    for (int r = 0; r < VIS_RPW; ++r) dot[r] = cadd[r] = 0.f;
    if (PROJ) {
        // straight-line loads on clamped indices like the rows above: all of them are in flight together
        const int n4h = a.pH >> 2;
        const size_t r_img = (size_t)max(a.src.vp[b], 0) * V, r_loc = (size_t)a.src.view[b] * V;
        float4 hv[PRJ_CPL];
#pragma unroll
        for (int i = 0; i < PRJ_CPL; ++i) {
            const int c = lane + 64 * i;
            const float4 t = reinterpret_cast<const float4*>(a.vec + (size_t)b * a.ldvec)[min(c, n4h - 1)];
            hv[i] = c < n4h ? t : f4zero();
        }
#pragma unroll
        for (int r = 0; r < VIS_RPW; ++r) {
            const int v = min(g * VSP_RPG + wave * VIS_RPW + r, V - 1);
            const float* pr = a.pv + (r_img + v) * (size_t)a.ldp;
            const float* lr = a.lv + (r_loc + v) * (size_t)a.ldp;
#pragma unroll
            for (int i = 0; i < PRJ_CPL; ++i) {
                const int cc = min(lane + 64 * i, n4h - 1);
                float4 t = reinterpret_cast<const float4*>(pr)[cc];
                f4add(t, reinterpret_cast<const float4*>(lr)[cc]);
                dot[r] += dot4(t, hv[i]);                          // (hv is zero beyond H)
            }
            cadd[r] = pr[a.pH] + lr[a.pH];
        }
    } else {
#pragma unroll
    for (int i = 0; i < VIS_CPL; ++i) {
        const int c = lane + 64 * i;
        const float4 q = c < n4 ? reinterpret_cast<const float4*>(a.vec + (size_t)b * a.ldvec)[c]
                                : f4zero();
#pragma unroll
        for (int r = 0; r < VIS_RPW; ++r) dot[r] += dot4(x[r][i], q);
    }
    }
#pragma unroll
    for (int r = 0; r < VIS_RPW; ++r) {
        float sw = wave_sum(dot[r]);
        if (PROJ) sw = prow.zero ? 0.f : sw + cadd[r];            // (an all-zero panorama scores 0 everywhere, as x . q does)
        const int vl = wave * VIS_RPW + r;
        if (lane == 0) s_score[vl] = (g * VSP_RPG + vl < V) ? sw : -INFINITY;
    }
    __syncthreads();
    vis_stamp(sp, b * VSP_G + g, 1);
    s = lane < VSP_RPG ? s_score[lane] : -INFINITY;
    m = wave_max(s);
    e = s > -INFINITY ? expf(s - m) : 0.f;
    }
    const float l = wave_sum(e);

    float4 p[VIS_CPL];
#pragma unroll
    for (int i = 0; i < VIS_CPL; ++i) p[i] = f4zero();
#pragma unroll
    for (int r = 0; r < VIS_RPW; ++r) {
        const float er = __shfl(e, wave * VIS_RPW + r, WAVE);
#pragma unroll
        for (int i = 0; i < VIS_CPL; ++i) f4fma(p[i], er, x[r][i]);
    }
    // publish the partials WRITE-THROUGH (sc1: straight to the memory side, visible to every XCD),
    // drain, then draw a ticket: no release fence (a buffer_wbl2 of the whole L2 costs far more
    // than this kernel), and the merging block reads them back with sc1 loads: no acquire fence.
    if (PHASE == 1) {                                            // next launch reads them
        block_row_sum<VIS_CPL, VSP_NW, VSP_SLOTS>(p, slots, n4, [&](int c, float4 t) {
            reinterpret_cast<float4*>(rec)[c] = t;
        });
        if (wave == 0) {
            if (lane < 32) rec[F + lane] = s;
            if (lane == 0) {
                rec[F + 32] = m;
                rec[F + 33] = l;
            }
        }
        vis_stamp(sp, b * VSP_G + g, 2);
        return;
    }
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(rec, 0, pstride * 4, 0x00020000);
    block_row_sum<VIS_CPL, VSP_NW, VSP_SLOTS>(p, slots, n4, [&](int c, float4 t) {
        const v4u v{__float_as_uint(t.x), __float_as_uint(t.y), __float_as_uint(t.z), __float_as_uint(t.w)};
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, c * 16, 0, 16);
    });
    if (wave == 0) {
        if (lane < 32) __hip_atomic_store(rec + F + lane, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) {
            __hip_atomic_store(rec + F + 32, F64 ? __int_as_float(__double2hiint(md)) : m, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(rec + F + 33, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (F64)
                __hip_atomic_store(rec + F + 34, __int_as_float(__double2loint(md)), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // EVERY storing wave drains
    __syncthreads();
    if (tid == 0)
        s_last = (__hip_atomic_fetch_add(sp.counter + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &
                  (unsigned)(VSP_G - 1)) == (unsigned)(VSP_G - 1);
    __syncthreads();
    if (!s_last) return;
    }   // PHASE != 2

    float* r0 = sp.part + (size_t)b * VSP_G * pstride;
    auto ldf = [&](float* q) {
        return PHASE == 0 ? __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *q;
    };
    float mg[VSP_G], lg[VSP_G];
    float dm[VSP_G];                                             // F64: m_k - M formed in float64
#pragma unroll
    for (int k = 0; k < VSP_G; ++k) {
        mg[k] = ldf(r0 + (size_t)k * pstride + F + 32);
        lg[k] = ldf(r0 + (size_t)k * pstride + F + 33);
    }
    float M = mg[0];
    if (F64) {
        double m64[VSP_G];
#pragma unroll
        for (int k = 0; k < VSP_G; ++k)
            m64[k] = __hiloint2double(__float_as_int(mg[k]), __float_as_int(ldf(r0 + (size_t)k * pstride + F + 34)));
        double M64 = m64[0];
#pragma unroll
        for (int k = 1; k < VSP_G; ++k) M64 = fmax(M64, m64[k]);
#pragma unroll
        for (int k = 0; k < VSP_G; ++k) dm[k] = (float)(m64[k] - M64);       // 0 for the maximal group, -inf for an empty one
    } else {
#pragma unroll
        for (int k = 1; k < VSP_G; ++k) M = fmaxf(M, mg[k]);
#pragma unroll
        for (int k = 0; k < VSP_G; ++k) dm[k] = mg[k] - M;
    }
    float kk[VSP_G], L = 0.f;                                    // m = -inf (empty group): c = 0, l = 0
#pragma unroll
    for (int k = 0; k < VSP_G; ++k) {
        kk[k] = expf(dm[k]);
        L += lg[k] * kk[k];
    }
    const float inv = 1.0f / L;
    if (tid < V) {
        const int gk = tid / VSP_RPG;
        const float sc = ldf(r0 + (size_t)gk * pstride + F + (tid - gk * VSP_RPG));
        // (F64: sc is relative to its group's maximum: sc + dm = score - M, both parts small and exact)
        a.alpha[(size_t)b * V + tid] = (F64 ? expf(sc + dm[gk]) : expf(sc - M)) * inv;
    }
#pragma unroll
    for (int k = 0; k < VSP_G; ++k) kk[k] *= inv;
    float* orow = a.out + (size_t)b * a.ldo;
    const Dropout dr = a.drop;
    const uint32_t rkey = drop_key(dr, (uint32_t)(dr.row0 + b));
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(r0, 0, VSP_G * pstride * 4, 0x00020000);
    for (int c = tid; c < n4; c += VSP_NW * 64) {
        v4u pk[VSP_G];
#pragma unroll
        for (int k = 0; k < VSP_G; ++k)
            pk[k] = __builtin_amdgcn_raw_buffer_load_b128(rs0, k * pstride * 4 + c * 16, 0, PHASE == 0 ? 16 : 0);
        float4 t = f4zero();
#pragma unroll
        for (int k = 0; k < VSP_G; ++k) {
            t.x += kk[k] * __uint_as_float(pk[k].x);
            t.y += kk[k] * __uint_as_float(pk[k].y);
            t.z += kk[k] * __uint_as_float(pk[k].z);
            t.w += kk[k] * __uint_as_float(pk[k].w);
        }
        if (dr.on()) {
            const uint32_t col = (uint32_t)(a.drop_col0 + 4 * c);
            t.x = dropout_keep(rkey, col + 0, dr.thresh) ? t.x * dr.scale : 0.f;
            t.y = dropout_keep(rkey, col + 1, dr.thresh) ? t.y * dr.scale : 0.f;
            t.z = dropout_keep(rkey, col + 2, dr.thresh) ? t.z * dr.scale : 0.f;
            t.w = dropout_keep(rkey, col + 3, dr.thresh) ? t.w * dr.scale : 0.f;
        }
        reinterpret_cast<float4*>(orow)[c] = t;
    }
}

template <bool H16>
__global__ __launch_bounds__(VSP_NW * 64) void visual_attn_split_kernel(VisArgs a, VisSplit sp) {
    visual_split_body<0, false, H16>(a, sp, blockIdx.x, blockIdx.y);
}
// the whole split attention on PROJECTED rows as a launch of its own (step 0's head of the projected chain: vec = h_init)
__global__ __launch_bounds__(VSP_NW * 64) void visual_attn_split_proj_kernel(VisArgs a, VisSplit sp) {
    visual_split_body<0, false, false, true>(a, sp, blockIdx.x, blockIdx.y);
}
template <bool H16>
__global__ __launch_bounds__(VSP_NW * 64) void visual_attn_split_f64_kernel(VisArgs a, VisSplit sp) {
    visual_split_body<0, true, H16>(a, sp, blockIdx.x, blockIdx.y);
}

// -------------------------------------------------------------------------------------------------
// The partials of the projected decode chain as a body of their own (launch (1), pair_proj_textfold_kernel<R, true>;
// merged by proj_merge_body in launch (2)).  visual_split_body<1, .., PROJ> keeps three rows, their accumulators and the
// projected rows of three views per wave: ~190 registers per lane, one 512-thread workgroup per CU for EVERY block of the
// grid it is compiled into.  This body fits 128 registers, so a CU holds two workgroups and the text groups of the same
// grid fill the slots the attention blocks leave:
//   - a row wave owns TWO rows (72 registers of row data) and forms the weighted sum in the first row's registers;
//   - it never holds a projected row: the block's other two waves (which visual_split_body sends home at once) form the
//     group's scores from the projected rows while the feature rows are on their way;
//   - a lane's nine chunks of a row are TYPED per slot, not per lane: slots [0, NI) are image chunks lane + 64 i, the
//     rest location chunks lane + 64 (i - NI).  Row and table are wave-uniform, so every load is a scalar base plus one
//     32-bit lane offset (the per-lane select between two 64-bit addresses of pano_load cost ~40 registers here and the
//     compiler then made the loads wait for one another).  Needs ceil(I4 / 64) + ceil(L4 / 64) <= VIS_CPL
//     (proj_partials_supported; the launcher declines otherwise and the partials ride in launch (2)).
// Nothing is masked on the way in: indices are clamped, a slot position past its part is never emitted, a view past V
// has weight e = 0 (feature values are finite), a padded sample's weights are zeroed for the sum alone.
// A sample is PPB_G = 3 groups of 12 views (V <= 36); the record of a group is laid out as visual_split_body's
// (P | scores | m, l), a group beyond V is (0 | -inf.. | -inf, 0) and merges to weight 0.  Plain stores: the kernel
// boundary is the hand-off, there is no ticket, so the group count need be no power of two.  No trace stamps
// (sf_debug_trace buffers are sized for VSP_G blocks per sample).
// -------------------------------------------------------------------------------------------------
constexpr int PPB_NW = 6, PPB_RPW = 2, PPB_RPG = PPB_NW * PPB_RPW, PPB_SLOTS = 3;
constexpr int PPB_SW = SMALL_WAVES - PPB_NW, PPB_SPW = PPB_RPG / PPB_SW;   // score waves, views scored per score wave
static_assert(PPB_G * PPB_RPG >= VSP_G * VSP_RPG, "covers every V the split attention takes");
static_assert(PPB_RPG <= 32, "a group's scores live in 32 record slots");
static_assert(PPB_SW >= 1 && PPB_SW * PPB_SPW == PPB_RPG, "the score waves share a group's views evenly");

// Every thread of a SMALL_WAVES * 64 block must call this (it synchronises).
__device__ __forceinline__ void proj_partials_body(const VisArgs& a, const VisSplit& sp, int g, int b) {
    __shared__ float4 slots[PPB_SLOTS][VIS_CPL * 64];
    __shared__ float s_score[PPB_RPG];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (uniform to the compiler too: scalar row addresses)
    const int V = a.src.V, I4 = a.src.IMG >> 2, L4 = a.src.LOC >> 2;
    const int F = a.src.IMG + a.src.LOC;
    const int NI = (I4 + 63) >> 6;
    float* rec = sp.part + ((size_t)b * PPB_G + g) * (F + 64);
    const int vp = a.src.vp[b], view = a.src.view[b];
    const bool zero = vp < 0;                                      // padded sample: all-zero panorama

    float4 x[PPB_RPW][VIS_CPL];
    if (wave < PPB_NW) {
        // ---- row waves: every load of both rows in flight at once
        const float4* img = reinterpret_cast<const float4*>(a.src.table) + (size_t)max(vp, 0) * V * I4;
        const float4* loc = reinterpret_cast<const float4*>(a.src.loc_table) + (size_t)view * V * L4;
#pragma unroll
        for (int r = 0; r < PPB_RPW; ++r) {
            const int v = min(g * PPB_RPG + wave * PPB_RPW + r, V - 1);
            const float4* ri = img + (size_t)v * I4;
            const float4* rl = L4 ? loc + (size_t)v * L4 : ri;     // (no location part: those slots are never emitted)
            const int nl = L4 ? L4 : I4;
#pragma unroll
            for (int i = 0; i < VIS_CPL; ++i) {
                const bool im = i < NI;
                const float4* base = im ? ri : rl;
                const int at = min(lane + 64 * (im ? i : i - NI), (im ? I4 : nl) - 1);
                x[r][i] = base[at];
            }
        }
    } else {
        // ---- score waves: score_v = (PV[row_v][:H] + LV[view * V + v][:H]) . h1 + PV[row_v][H] + LV[..][H]
        const int n4h = a.pH >> 2;
        const size_t r_img = (size_t)max(vp, 0) * V, r_loc = (size_t)view * V;
        float4 hv[PRJ_CPL], pj[PPB_SPW][PRJ_CPL], lj[PPB_SPW][PRJ_CPL];
        // (the constants at column H: lane r fetches view r's, one load per table instead of a register per view)
        const int vc = min(g * PPB_RPG + (wave - PPB_NW) * PPB_SPW + min(lane, PPB_SPW - 1), V - 1);
        const float cst = a.pv[(r_img + vc) * (size_t)a.ldp + a.pH] + a.lv[(r_loc + vc) * (size_t)a.ldp + a.pH];
#pragma unroll
        for (int i = 0; i < PRJ_CPL; ++i)
            hv[i] = reinterpret_cast<const float4*>(a.vec + (size_t)b * a.ldvec)[min(lane + 64 * i, n4h - 1)];
#pragma unroll
        for (int r = 0; r < PPB_SPW; ++r) {
            const int v = min(g * PPB_RPG + (wave - PPB_NW) * PPB_SPW + r, V - 1);
            const float* pr = a.pv + (r_img + v) * (size_t)a.ldp;
            const float* lr = a.lv + (r_loc + v) * (size_t)a.ldp;
#pragma unroll
            for (int i = 0; i < PRJ_CPL; ++i) {
                const int cc = min(lane + 64 * i, n4h - 1);
                pj[r][i] = reinterpret_cast<const float4*>(pr)[cc];
                lj[r][i] = reinterpret_cast<const float4*>(lr)[cc];
            }
        }
#pragma unroll
        for (int r = 0; r < PPB_SPW; ++r) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < PRJ_CPL; ++i) {
                float4 t = pj[r][i];
                f4add(t, lj[r][i]);
                d += (lane + 64 * i < n4h ? 1.f : 0.f) * dot4(t, hv[i]);      // (clamped lanes beyond H count for nothing)
            }
            // (an all-zero panorama scores 0 everywhere -- blended, not branched on: the loads above stay unconditional)
            const float sw = (zero ? 0.f : 1.f) * (wave_sum(d) + __shfl(cst, r, WAVE));
            const int vl = (wave - PPB_NW) * PPB_SPW + r;
            if (lane == 0) s_score[vl] = (g * PPB_RPG + vl < V) ? sw : -INFINITY;
        }
    }
    __syncthreads();
    const float s = lane < PPB_RPG ? s_score[lane] : -INFINITY;
    const float m = wave_max(s);                                   // -inf: the group lies beyond V
    const float e = s > -INFINITY ? expf(s - m) : 0.f;
    const float l = wave_sum(e);

    // the weighted sum in place: p = e0 x0 takes the first row's registers, the second row is folded into them
    float4 p[VIS_CPL];
    if (wave < PPB_NW) {
        const float ew = zero ? 0.f : e;
        const float e0 = __shfl(ew, wave * PPB_RPW, WAVE);
#pragma unroll
        for (int i = 0; i < VIS_CPL; ++i)
            p[i] = make_float4(e0 * x[0][i].x, e0 * x[0][i].y, e0 * x[0][i].z, e0 * x[0][i].w);
#pragma unroll
        for (int r = 1; r < PPB_RPW; ++r) {
            const float er = __shfl(ew, wave * PPB_RPW + r, WAVE);
#pragma unroll
            for (int i = 0; i < VIS_CPL; ++i) f4fma(p[i], er, x[r][i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < VIS_CPL; ++i) p[i] = f4zero();
    }
    // (slot position k = lane + 64 i of the sum is chunk k of the image part, or chunk k - 64 NI of the location part)
    block_row_sum<VIS_CPL, SMALL_WAVES, PPB_SLOTS>(p, slots, VIS_CPL * 64, [&](int k, float4 t) {
        const bool im = k < 64 * NI;
        const int c = im ? k : k - 64 * NI;
        if (c < (im ? I4 : L4)) reinterpret_cast<float4*>(rec)[im ? c : I4 + c] = t;
    });
    if (wave == 0) {
        if (lane < 32) rec[F + lane] = s;
        if (lane == 0) {
            rec[F + 32] = m;
            rec[F + 33] = l;
        }
    }
}

// The merge of proj_partials_body's G records per sample (RPG views each) into alpha [V] and the normalised weighted sum:
// visual_split_body<2> on another record count.  Plain loads (the records come from the launch before); no barrier, so
// every thread of the block takes part.
template <int G, int RPG>
__device__ __forceinline__ void proj_merge_body(const VisArgs& a, const VisSplit& sp, int b) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x;
    const int V = a.src.V;
    const int F = a.src.IMG + a.src.LOC, n4 = F >> 2;
    const int pstride = F + 64;
    float* r0 = sp.part + (size_t)b * G * pstride;
    float mg[G], kk[G];
#pragma unroll
    for (int k = 0; k < G; ++k) mg[k] = r0[(size_t)k * pstride + F + 32];
    float M = mg[0];                                             // (group 0 is never empty)
#pragma unroll
    for (int k = 1; k < G; ++k) M = fmaxf(M, mg[k]);
    float L = 0.f;                                               // m = -inf (empty group): weight 0, l = 0
#pragma unroll
    for (int k = 0; k < G; ++k) {
        kk[k] = expf(mg[k] - M);
        L += r0[(size_t)k * pstride + F + 33] * kk[k];
    }
    const float inv = 1.0f / L;
    if (tid < V) {
        const int gk = tid / RPG;
        const float sc = r0[(size_t)gk * pstride + F + (tid - gk * RPG)];
        a.alpha[(size_t)b * V + tid] = expf(sc - M) * inv;
    }
#pragma unroll
    for (int k = 0; k < G; ++k) kk[k] *= inv;
    float* orow = a.out + (size_t)b * a.ldo;
    const Dropout dr = a.drop;
    const uint32_t rkey = drop_key(dr, (uint32_t)(dr.row0 + b));
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(r0, 0, G * pstride * 4, 0x00020000);
    for (int c = tid; c < n4; c += SMALL_WAVES * 64) {
        v4u pk[G];
#pragma unroll
        for (int k = 0; k < G; ++k) pk[k] = __builtin_amdgcn_raw_buffer_load_b128(rs0, k * pstride * 4 + c * 16, 0, 0);
        float4 t = f4zero();
#pragma unroll
        for (int k = 0; k < G; ++k) {
            t.x += kk[k] * __uint_as_float(pk[k].x);
            t.y += kk[k] * __uint_as_float(pk[k].y);
            t.z += kk[k] * __uint_as_float(pk[k].z);
            t.w += kk[k] * __uint_as_float(pk[k].w);
        }
        if (dr.on()) {
            const uint32_t col = (uint32_t)(a.drop_col0 + 4 * c);
            t.x = dropout_keep(rkey, col + 0, dr.thresh) ? t.x * dr.scale : 0.f;
            t.y = dropout_keep(rkey, col + 1, dr.thresh) ? t.y * dr.scale : 0.f;
            t.z = dropout_keep(rkey, col + 2, dr.thresh) ? t.z * dr.scale : 0.f;
            t.w = dropout_keep(rkey, col + 3, dr.thresh) ? t.w * dr.scale : 0.f;
        }
        // (gate-space rows, block-uniform: the 4H part is the next cell's addend, the location part stays an input)
        float4* dst = reinterpret_cast<float4*>(orow) + c;
        if (a.out_img) {
            const int i4 = a.src.IMG >> 2;
            dst = c < i4 ? reinterpret_cast<float4*>(a.out_img + (size_t)b * a.ld_img) + c : reinterpret_cast<float4*>(orow) + (c - i4);
        }
        *dst = t;
    }
}

// =================================================================================================
// Text / path-context attention core (model.py:129-139): L rows of H floats, CPL = 2 (H <= 512).
// forward : s_l = ctx_l . t (masked -> -inf), alpha = softmax, wc = sum alpha_l ctx_l
// backward: d_l = ctx_l . dwc, ds_l = alpha_l (d_l - sum alpha d), dt = sum ds_l ctx_l,
//           dctx_l += alpha_l dwc + ds_l t
// =================================================================================================

struct TxtArgs {
    const float* ctx;      // [B, L, H]
    const uint8_t* mask;   // [B, L] or null
    int L, H;
    const float* vec;      // fwd: t [B, ldvec]; bwd: dwc [B, ldvec]
    int ldvec;
    const float* vec2;     // bwd: t [B, ldvec2]
    int ldvec2;
    float* alpha;          // [B, L]
    float* out;            // fwd: wc [B, ldo]; bwd: dt [B, ldo]
    int ldo;
    float* dctx;           // bwd, accumulated; may be null
    const int32_t* ctx_row;  // fwd: sample b attends over ctx / mask row ctx_row[b] (null = b)
    float* ds_out;         // bwd, optional [B, L]: the score gradients (for a deferred dctx update)
};

template <int RPW, int MODE, int NW = TXT_NW>
__device__ __forceinline__ void text_attn_body(const TxtArgs& a, int b) {
    __shared__ float4 slots[TXT_SLOTS][TXT_CPL * 64];
    __shared__ float s_score[NW * RPW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = a.L, n4 = a.H >> 2;
    const int bc = a.ctx_row ? a.ctx_row[b] : b;
    const float4* ctx = reinterpret_cast<const float4*>(a.ctx) + (size_t)bc * L * n4;

    // straight-line loads (clamped indices, value selects): a load inside a branch costs a full
    // memory round trip each (see sf_rows.h)
    float4 x[RPW][TXT_CPL];
    uint8_t mk[RPW];
    // the mask bytes are loaded UNCONDITIONALLY (from the context itself when there is no mask): a load
    // behind even a block-uniform branch is followed by a full `s_waitcnt vmcnt(0)`, which made every
    // context row its own memory round trip
    const bool use_mask = MODE == 0 && a.mask != nullptr;
    const uint8_t* mrow = use_mask ? a.mask + (size_t)bc * L : reinterpret_cast<const uint8_t*>(ctx);
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int l = wave * RPW + r;
        const int lc = min(l, L - 1);
#pragma unroll
        for (int i = 0; i < TXT_CPL; ++i) {
            const int c = lane + 64 * i;
            const float4 t = ctx[(size_t)lc * n4 + min(c, n4 - 1)];
            x[r][i] = (l < L && c < n4) ? t : f4zero();
        }
        mk[r] = mrow[lc];
    }
    float4 v1[TXT_CPL], v2[TXT_CPL];
#pragma unroll
    for (int i = 0; i < TXT_CPL; ++i) {
        const int c = lane + 64 * i;
        const int cc = min(c, n4 - 1);
        const float4 t1 = reinterpret_cast<const float4*>(a.vec + (size_t)b * a.ldvec)[cc];
        v1[i] = c < n4 ? t1 : f4zero();
        v2[i] = f4zero();
        if (MODE == 1) {
            const float4 t2 = reinterpret_cast<const float4*>(a.vec2 + (size_t)b * a.ldvec2)[cc];
            v2[i] = c < n4 ? t2 : f4zero();
        }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < TXT_CPL; ++i) d += dot4(x[r][i], v1[i]);
        d = wave_sum(d);
        const int l = wave * RPW + r;
        if (lane == 0 && l < L) s_score[l] = (use_mask && mk[r]) ? -INFINITY : d;
    }
    __syncthreads();

    // L <= 128: lane holds entries lane and lane + 64
    const int l0 = lane, l1 = lane + 64;
    float w0, w1;
    if (MODE == 0) {
        const float s0 = l0 < L ? s_score[l0] : -INFINITY;
        const float s1 = l1 < L ? s_score[l1] : -INFINITY;
        const float m = wave_max(fmaxf(s0, s1));
        const float e0 = l0 < L ? expf(s0 - m) : 0.f;
        const float e1 = l1 < L ? expf(s1 - m) : 0.f;
        const float inv = 1.0f / wave_sum(e0 + e1);
        w0 = e0 * inv;
        w1 = e1 * inv;
        if (wave == 0) {
            if (l0 < L) a.alpha[(size_t)b * L + l0] = w0;
            if (l1 < L) a.alpha[(size_t)b * L + l1] = w1;
        }
    } else {
        const float t0 = a.alpha[(size_t)b * L + min(l0, L - 1)];
        const float t1 = a.alpha[(size_t)b * L + min(l1, L - 1)];
        const float a0 = l0 < L ? t0 : 0.f;
        const float a1 = l1 < L ? t1 : 0.f;
        const float d0 = l0 < L ? s_score[l0] : 0.f;
        const float d1 = l1 < L ? s_score[l1] : 0.f;
        const float tot = wave_sum(a0 * d0 + a1 * d1);
        w0 = a0 * (d0 - tot);
        w1 = a1 * (d1 - tot);
        if (a.ds_out && wave == 0) {                             // block-uniform
            if (l0 < L) a.ds_out[(size_t)b * L + l0] = w0;
            if (l1 < L) a.ds_out[(size_t)b * L + l1] = w1;
        }
    }

    float4 p[TXT_CPL];
#pragma unroll
    for (int i = 0; i < TXT_CPL; ++i) p[i] = f4zero();
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int l = wave * RPW + r;
        const int src = (l < L ? l : 0) & 63;
        const float lo = __shfl(w0, src, WAVE), hi = __shfl(w1, src, WAVE);
        const float wr = (l < 64) ? lo : hi;
        const float wl = l < L ? wr : 0.f;                       // x is zero beyond L anyway
#pragma unroll
        for (int i = 0; i < TXT_CPL; ++i) f4fma(p[i], wl, x[r][i]);
    }
    if (MODE == 1 && a.dctx) {                                   // dctx_l += alpha_l dwc + ds_l t
        float4 g[RPW][TXT_CPL];
        float al[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {                          // all read-modify-write loads first
            const int lc = min(wave * RPW + r, L - 1);
            al[r] = a.alpha[(size_t)b * L + lc];
            const float4* drow = reinterpret_cast<const float4*>(a.dctx) + ((size_t)b * L + lc) * n4;
#pragma unroll
            for (int i = 0; i < TXT_CPL; ++i) g[r][i] = drow[min(lane + 64 * i, n4 - 1)];
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int l = wave * RPW + r;
            const int src = (l < L ? l : 0) & 63;
            const float lo = __shfl(w0, src, WAVE), hi = __shfl(w1, src, WAVE);
            const float wr = (l < 64) ? lo : hi;
            float4* drow = reinterpret_cast<float4*>(a.dctx) + ((size_t)b * L + min(l, L - 1)) * n4;
#pragma unroll
            for (int i = 0; i < TXT_CPL; ++i) {
                const int c = lane + 64 * i;
                f4fma(g[r][i], al[r], v1[i]);
                f4fma(g[r][i], wr, v2[i]);
                if (l < L && c < n4) drow[c] = g[r][i];
            }
        }
    }
    float* orow = a.out + (size_t)b * a.ldo;
    block_row_sum<TXT_CPL, NW, TXT_SLOTS>(p, slots, n4, [&](int c, float4 t) {
        reinterpret_cast<float4*>(orow)[c] = t;
    });
}

template <int RPW, int MODE>
__global__ __launch_bounds__(TXT_NW * 64) void text_attn_kernel(TxtArgs a) {
    text_attn_body<RPW, MODE>(a, blockIdx.x);
}

// =================================================================================================
// Candidate scoring (model.py:342-352 after folding): one wave per candidate, A <= 16.
// forward : logit[b,a] = u_a . r[b] + (wt[b] . b_a + b_out)
// backward: dr[b] = sum_a dlogit[b,a] u_a ;  dc[b] = sum_a dlogit[b,a]
// =================================================================================================

struct ScoreArgs {
    CandSrc src;
    int ldr;               // row stride of r
    const float* cst;      // optional per-row constant (stride ldr); null -> wt.b_a + b_out
    const float* r;        // fwd [B,ldr]
    const float* wt;       // fwd [B,D]
    const float* b_a;      // [D]
    const float* b_out;    // [1]
    int D;
    float* logit;          // fwd out [B,A]; bwd: dlogit in
    float* dr;             // bwd out [B,F]
    float* dc;             // bwd out [B]
    CeSrc ce;              // bwd: ce.logit != null -> d(logit) is formed here (and stored to `logit`)
};

// wt[b] . b_a + b_out (or the precomputed per-row constant): straight-line loads for D <= 256
__device__ __forceinline__ float score_const(const ScoreArgs& a, int b, int lane) {
    if (a.cst) return a.cst[(size_t)b * a.ldr];                  // block-uniform
    float c = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = lane + 64 * i;
        const float w = a.wt[(size_t)b * a.D + min(k, a.D - 1)] * a.b_a[min(k, a.D - 1)];
        c += k < a.D ? w : 0.f;
    }
    for (int k = lane + 256; k < a.D; k += 64) c += a.wt[(size_t)b * a.D + k] * a.b_a[k];
    return wave_sum(c) + a.b_out[0];
}

template <bool H16>
__global__ __launch_bounds__(SC_NW * 64) void score_fwd_kernel(ScoreArgs a) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int A = a.src.A;
    if (wave >= A) return;
    const int n4 = (a.src.IMG + a.src.LOC) >> 2;
    const CandRow row = cand_row<H16>(a.src, b, wave);
    const float4* rv = reinterpret_cast<const float4*>(a.r + (size_t)b * a.ldr);
    float4 x[SC_CPL], q[SC_CPL];
#pragma unroll
    for (int i = 0; i < SC_CPL; ++i) x[i] = f4zero();
    if (!row.zero) {        // wave-uniform: stop / padding rows cost no traffic; one block of loads
#pragma unroll
        for (int i = 0; i < SC_CPL; ++i) {
            const int c = lane + 64 * i;
            x[i] = cand_load<H16>(row, c, c < n4, n4);
            q[i] = rv[min(c, n4 - 1)];
        }
    }
    float d = 0.f;
    if (!row.zero) {
#pragma unroll
        for (int i = 0; i < SC_CPL; ++i) d += dot4(x[i], q[i]);  // x is zero beyond n4
    }
    const float cst = score_const(a, b, lane);
    d = wave_sum(d);
    if (lane == 0) a.logit[(size_t)b * A + wave] = d + cst;
}

// Scoring + per-step glue fused (one dependent stage instead of two): wave a keeps candidate a's row
// in registers, the 16 logits meet in LDS, wave 0 masks / soft-maxes / picks the action, and the wave
// that owns the chosen row writes dropout(u_next) straight into the next step's LSTM input.
template <bool H16 = false>
__device__ __forceinline__ void score_glue_body(const ScoreArgs& a, const FGlue& g, int b) {
    __shared__ float s_logit[64];
    __shared__ int s_at;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int A = a.src.A;
    const int n4 = (a.src.IMG + a.src.LOC) >> 2;
    const CandRow row = cand_row<H16>(a.src, b, wave);
    const FGlueIn gin = follower_glue_load(g, b);               // (used by wave 0; cheap for the rest)
    const float4* rv = reinterpret_cast<const float4*>(a.r + (size_t)b * a.ldr);
    float4 x[SC_CPL], q[SC_CPL];
#pragma unroll
    for (int i = 0; i < SC_CPL; ++i) x[i] = f4zero();
    const bool have = wave < A && !row.zero;   // wave-uniform: stop / padding rows cost no traffic
    if (have) {
#pragma unroll
        for (int i = 0; i < SC_CPL; ++i) {
            const int c = lane + 64 * i;
            x[i] = cand_load<H16>(row, c, c < n4, n4);
            q[i] = rv[min(c, n4 - 1)];
        }
    }
    float d = 0.f;
    if (have) {
#pragma unroll
        for (int i = 0; i < SC_CPL; ++i) d += dot4(x[i], q[i]);
    }
    const float cst = score_const(a, b, lane);
    d = wave_sum(d);
    if (lane == 0 && wave < A) s_logit[wave] = d + cst;
    __syncthreads();
    if (wave == 0) {
        const int at = follower_glue_row(g, b, lane < A ? s_logit[lane] : 0.f, gin);
        if (lane == 0) s_at = at;
        if (g.nav.on && lane < A) nav_advance_slot(g.nav, b, lane, at, gin.was_ended || at == 0);
    }
    __syncthreads();
    if (g.u_next && wave == s_at) {
#pragma unroll
        for (int i = 0; i < SC_CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < n4) store_u_next(g, b, c, x[i]);
        }
    }
}

template <bool H16>
__global__ __launch_bounds__(SC_NW * 64) void score_glue_kernel(ScoreArgs a, FGlue g) { score_glue_body<H16>(a, g, blockIdx.x); }

template <bool H16>
__global__ __launch_bounds__(SC_NW * 64) void score_bwd_kernel(ScoreArgs a) {
    __shared__ float4 slots[SC_SLOTS][SC_CPL * 64];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int A = a.src.A;
    const int n4 = (a.src.IMG + a.src.LOC) >> 2;
    float w, dlv;
    if (a.ce.logit) {                                            // block-uniform: fused CE backward
        const int64_t tgt = a.ce.target[b];
        const float lg = a.ce.logit[(size_t)b * a.ce.ld + min(lane, A - 1)];
        const float l = lane < A ? lg : -INFINITY;
        const float m = wave_max(l);
        const float e = l > -INFINITY ? expf(l - m) : 0.f;
        const float ssum = wave_sum(e);
        const float gs = a.ce.gscale[0];
        dlv = (tgt == a.ce.ignore || lane >= A) ? 0.f : gs * (e / ssum - (lane == (int)tgt ? 1.f : 0.f));
        if (wave == 0 && lane < A) a.logit[(size_t)b * A + lane] = dlv;
        w = __shfl(dlv, min(wave, A - 1), WAVE);
    } else {
        w = a.logit[(size_t)b * A + min(wave, A - 1)];
        dlv = a.logit[(size_t)b * A + min(lane, A - 1)];
    }
    const CandRow row = cand_row<H16>(a.src, b, wave);
    float4 p[SC_CPL];
#pragma unroll
    for (int i = 0; i < SC_CPL; ++i) p[i] = f4zero();
    if (wave < A && !row.zero && w != 0.f) {                     // wave-uniform
#pragma unroll
        for (int i = 0; i < SC_CPL; ++i) {
            const int c = lane + 64 * i;
            f4fma(p[i], w, cand_load<H16>(row, c, c < n4, n4));
        }
    }
    if (wave == 0) {
        const float tot = wave_sum(lane < A ? dlv : 0.f);
        if (lane == 0) a.dc[b] = tot;
    }
    float* orow = a.dr + (size_t)b * (n4 << 2);
    block_row_sum<SC_CPL, SC_NW, SC_SLOTS>(p, slots, n4, [&](int c, float4 t) {
        reinterpret_cast<float4*>(orow)[c] = t;
    });
}

// =================================================================================================
// Paired launches.  A decode step is a chain of dependent, latency-bound kernels that each use a
// fraction of the chip; the visual half of step t+1 (t_v, q, visual attention: needs only h1 of
// step t) is independent of the text / scoring half of step t.  Two hipGraph branches (or streams)
// need a fork and a join per step, which cost more than the overlap gains (724K vs 815K agent-steps/s
// measured), so two independent kernels share ONE grid:
// blocks [0, nA) run body A, the rest body B.  Threads beyond a body's block size exit at once
// (whole waves: a workgroup barrier only counts live waves).
// =================================================================================================
template <int MTA, int CPWA, int MTB, int CPWB>
__global__ __launch_bounds__(SMALL_WAVES * 64) void pair_small_small_kernel(SmallArgs a, int gxa,
                                                                           int na, SmallArgs b,
                                                                           int gxb) {
    const int bid = blockIdx.x;
    if (bid < na)
        small_gemm_body<MTA, CPWA>(a, bid % gxa, bid / gxa);
    else
        small_gemm_body<MTB, CPWB>(b, (bid - na) % gxb, (bid - na) / gxb);
}

template <int MT, int CPW, int RPW>
__global__ __launch_bounds__(TXT_NW * 64) void pair_small_text_kernel(SmallArgs a, int gxa, int na,
                                                                      TxtArgs t) {
    const int bid = blockIdx.x;
    if (bid < na) {
        if (threadIdx.x >= SMALL_WAVES * 64) return;
        small_gemm_body<MT, CPW>(a, bid % gxa, bid / gxa);
    } else {
        text_attn_body<RPW, 0>(t, bid - na);
    }
}

// (APRO is false in every instantiation since the three-launch folded chain went; the parameter stays because it is part
//  of the surviving kernels' symbol names -- DESIGN.md, "Retired experiments", follow-up)
template <int MT, int CPW, int PHASE, bool APRO = false, bool H16 = false>
__global__ __launch_bounds__(SMALL_WAVES * 64) void pair_vis_small_kernel(VisArgs v, VisSplit sp,
                                                                         int nv, SmallArgs b,
                                                                         int gxb) {
    const int bid = blockIdx.x;
    if (bid < nv) {
        if (threadIdx.x >= VSP_NW * 64) return;
        if (PHASE == 2)
            visual_split_body<2>(v, sp, 0, bid);
        else
            visual_split_body<PHASE, false, H16>(v, sp, bid % VSP_G, bid / VSP_G);
    } else {
        small_gemm_body<MT, CPW, false, APRO>(b, (bid - nv) % gxb, (bid - nv) / gxb);
    }
}


// scoring + glue of step t beside the merge of the attention partials of step t+1 (folded inference chain: the two
// halves of the next step's LSTM input -- u_next from the glue, the attended feature from the merge -- land in one launch)
// (H16 is the CANDIDATE table's storage: the phase-2 merge reads partials, never the table)
template <bool H16>
__global__ __launch_bounds__(SC_NW * 64) void pair_score_merge_kernel(ScoreArgs a, FGlue g, int nb, VisArgs v, VisSplit sp) {
    const int bid = blockIdx.x;
    if (bid < nb) {
        score_glue_body<H16>(a, g, bid);
    } else {
        if (threadIdx.x >= VSP_NW * 64) return;
        visual_split_body<2>(v, sp, 0, bid - nb);
    }
}


// =================================================================================================
// Scoring on PROJECTED candidate rows (the projected decode chain, sf_api_follower.hip: tail_proj).
// logit[b,a] = u_a . r + c with [r | c] = M_a h~ + c_a (sf_decoder_fold) re-associated to (u_a^T M_a) . h~ + u_a . c_a + c:
// the image part of the bracket is row (vp, cand_view) of PA -- candidate rows are rows of the same panoramas -- and the
// location part, four values each repeated LOC/4 times (cand_load), is sum_g sc_g LA[g].  LA[4] = [m | c0] is the
// constant row of the fold (c = m . h~ + c0), which is all a zero row (stop, padding, padded sample) gets.
// h~ = tanh(z + y) is formed here from the two buffers the A-prologue of the unprojected chains reads (apro_form).
// 8 waves, two candidate slots per wave (A <= 16): a projected row is 2 KB, so nothing about it is register-bound.
// The chosen action's UNPROJECTED row (the next gate product needs all of it) is gathered behind the choice.
// =================================================================================================
struct ProjScoreArgs {
    CandSrc src;
    const float* pa;       // [n_vp * V, ldp]: row n = [x_n^T M_a[:IMG, :] | x_n . c_a[:IMG]]
    const float* la;       // [5, ldp]: the four sin/cos groups of the location part, then [m | c0]
    int ldp, H;
    const float* z;        // [B, ldz] merged text-attention sum (text_fold_body)
    const float* y;        // [B, ldy] W_out[:, H:] h1
    int ldz, ldy;
    const float* gu;       // [n_vp * V, 4H] gate-space image rows (sf_gate_rows_build) or null
    const float* gl;       // [4, 4H]: the four sin/cos groups of the location part in gate space
    float* xg_next;        // [B, 4H]: the chosen action's row in gate space, for the next step's cell (null: not formed)
};

__device__ __forceinline__ void proj_score_glue_body(const ProjScoreArgs& a, const FGlue& g, int b) {
    constexpr int NW = SMALL_WAVES, SLOTS = 2;
    __shared__ float s_logit[64];
    __shared__ int s_at;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int A = a.src.A, V = a.src.V, H = a.H, n4h = H >> 2;
    const size_t ldp = (size_t)a.ldp;
    const FGlueIn gin = follower_glue_load(g, b);               // (used by wave 0; cheap for the rest)
    // every wave keeps the sample's candidate list with lane a holding candidate a: the slots below and the gather
    // behind the choice take theirs by shuffle, not by a second round trip
    const int vp = a.src.vp[b], an = a.src.a_num[b];
    const int cvl = a.src.cand_view[(size_t)b * A + min(lane, A - 1)];
    const float4 scl = reinterpret_cast<const float4*>(a.src.cand_sincos)[(size_t)b * A + min(lane, A - 1)];
    float4 zv[PRJ_CPL], yv[PRJ_CPL], lav[5][PRJ_CPL], pav[SLOTS][PRJ_CPL];
    float lac[5], pac[SLOTS];
#pragma unroll
    for (int i = 0; i < PRJ_CPL; ++i) {
        const int cc = min(lane + 64 * i, n4h - 1);
        zv[i] = reinterpret_cast<const float4*>(a.z + (size_t)b * a.ldz)[cc];
        yv[i] = reinterpret_cast<const float4*>(a.y + (size_t)b * a.ldy)[cc];
#pragma unroll
        for (int q = 0; q < 5; ++q) lav[q][i] = reinterpret_cast<const float4*>(a.la + q * ldp)[cc];
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) lac[q] = a.la[q * ldp + H];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const int view = __shfl(cvl, min(wave + NW * k, A - 1), WAVE);
        const float* pr = a.pa + ((size_t)max(vp, 0) * V + min(max(view, 0), V - 1)) * ldp;
#pragma unroll
        for (int i = 0; i < PRJ_CPL; ++i) pav[k][i] = reinterpret_cast<const float4*>(pr)[min(lane + 64 * i, n4h - 1)];
        pac[k] = pr[H];
    }
    float4 ht[PRJ_CPL];
#pragma unroll
    for (int i = 0; i < PRJ_CPL; ++i) ht[i] = lane + 64 * i < n4h ? apro_form(yv[i], zv[i]) : f4zero();
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const int ac = wave + NW * k, acc = min(ac, A - 1);
        const float s0 = __shfl(scl.x, acc, WAVE), s1 = __shfl(scl.y, acc, WAVE), s2 = __shfl(scl.z, acc, WAVE),
                    s3 = __shfl(scl.w, acc, WAVE);
        // (blended arithmetically, never branched on: rows are finite, a zero row keeps the constant row alone)
        const float hm = (ac < A && ac != 0 && ac < an && vp >= 0) ? 1.f : 0.f;
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < PRJ_CPL; ++i) {
            float4 w = pav[k][i];
            f4fma(w, s0, lav[0][i]);
            f4fma(w, s1, lav[1][i]);
            f4fma(w, s2, lav[2][i]);
            f4fma(w, s3, lav[3][i]);
            float4 t = lav[4][i];
            f4fma(t, hm, w);
            d += dot4(t, ht[i]);
        }
        d = wave_sum(d);
        const float cst = lac[4] + hm * (pac[k] + s0 * lac[0] + s1 * lac[1] + s2 * lac[2] + s3 * lac[3]);
        if (lane == 0 && ac < A) s_logit[ac] = d + cst;
    }
    __syncthreads();
    // The chosen row once more in GATE space (a.xg_next; sf_gate_rows_build): u W_ih[:, :F]^T = GU[vp V + view] +
    // sum_k sincos_k GL[k], zeros for a zero row.  One float4 per thread (H <= PRJ_CPL * 256, the block's threads:
    // proj_tables_fit).  The four GL chunks do not depend on the choice: asked for here, while wave 0 makes it.  Without a
    // target the same loads read the first chunk of LA: pointers and indices are selected, no load sits behind a branch.
    const bool gate = a.xg_next != nullptr;
    const int gc = gate ? min(tid, H - 1) : 0, gs = gate ? H : 0;
    const float4* glp = reinterpret_cast<const float4*>(gate ? a.gl : a.la);
    const float4 gl0 = glp[gc], gl1 = glp[gs + gc], gl2 = glp[2 * gs + gc], gl3 = glp[3 * gs + gc];
    if (wave == 0) {
        const int at = follower_glue_row(g, b, lane < A ? s_logit[lane] : 0.f, gin);
        if (lane == 0) s_at = at;
        if (g.nav.on && lane < A) nav_advance_slot(g.nav, b, lane, at, gin.was_ended || at == 0);
    }
    __syncthreads();
    const int at = min(max(s_at, 0), A - 1);
    const bool zero = at == 0 || at >= an || vp < 0;
    const int view = __shfl(cvl, at, WAVE);
    const float c0 = __shfl(scl.x, at, WAVE), c1 = __shfl(scl.y, at, WAVE), c2 = __shfl(scl.z, at, WAVE),
                c3 = __shfl(scl.w, at, WAVE);
    const size_t trow = (size_t)max(vp, 0) * V + min(max(view, 0), V - 1);
    // (the GU chunk ahead of the raw row's stores: both gathers are one round trip)
    float4 gw = (gate ? reinterpret_cast<const float4*>(a.gu) + trow * H : glp)[gc];
    if (g.u_next) {                                              // block-uniform
        const int n4 = (a.src.IMG + a.src.LOC) >> 2;
        CandRow row;
        row.zero = zero;
        row.I4 = a.src.IMG >> 2;
        row.g4 = max(a.src.LOC >> 4, 1);
        row.img = reinterpret_cast<const float4*>(a.src.table) + trow * row.I4;
        row.img16 = nullptr;
        row.s0 = c0; row.s1 = c1; row.s2 = c2; row.s3 = c3;
        for (int c = tid; c < n4; c += NW * 64) store_u_next(g, b, c, cand_load<false>(row, c, !row.zero, n4));
    }
    if (gate && tid < H) {
        f4fma(gw, c0, gl0);
        f4fma(gw, c1, gl1);
        f4fma(gw, c2, gl2);
        f4fma(gw, c3, gl3);
        reinterpret_cast<float4*>(a.xg_next)[(size_t)b * H + tid] = zero ? f4zero() : gw;
    }
}

// launch (2) of the projected chain: scoring + glue beside the attention of step t + 1 --
//   VPHASE 2: the merge of the PPB_G records per sample launch (1) left (proj_partials_body; the default placement);
//   VPHASE 0: partials, ticket and merge here (sf_debug_projected_partials_late: launch (1) is the text stage alone)
template <int VPHASE>
__global__ __launch_bounds__(SMALL_WAVES * 64) void pair_proj_score_kernel(ProjScoreArgs a, FGlue g, int nb, VisArgs v, VisSplit sp,
                                                                         int nv) {
    const int bid = blockIdx.x;
    if (VPHASE == 0) {                                           // (the long blocks first)
        if (bid >= nv) return proj_score_glue_body(a, g, bid - nv);
        if (threadIdx.x >= VSP_NW * 64) return;
        visual_split_body<0, false, false, true>(v, sp, bid % VSP_G, bid / VSP_G);
    } else {
        if (bid < nb) return proj_score_glue_body(a, g, bid);
        proj_merge_body<PPB_G, PPB_RPG>(v, sp, bid - nb);
    }
}

// Launch (2) with the NEXT step's recurrent gate product beside it: blocks [0, nh) run the small product
// xg_h = h1 W_hh^T + b_ih + b_hh (small_gemm_body<MT, 4> over the plan of [B, H] x [4H, H]^T: nothing in this launch reads
// it, and it reads nothing launches (1) or (2) write) behind the scoring + glue blocks [0, nb) and the merge blocks
// [nb, nb + nm).  The product blocks come LAST: measured at B = 100, 11.4 us per launch and 1.155 ms per rollout against
// 12.8 us and 1.180 ms with them first (profiles/recurrent_row_ab.txt) -- the scoring blocks' dependent load chain starts at
// once and the products fill in behind.  A kernel of its own: pair_proj_score_kernel<2> stays what it was for every step
// without the row.
template <int MT>
__global__ __launch_bounds__(SMALL_WAVES * 64) void pair_proj_score_hh_kernel(ProjScoreArgs a, FGlue g, int nb, VisArgs v, VisSplit sp,
                                                                            int nm, SmallArgs hh, int gxh) {
    const int bid = blockIdx.x;
    if (bid < nb) return proj_score_glue_body(a, g, bid);
    if (bid < nb + nm) return proj_merge_body<PPB_G, PPB_RPG>(v, sp, bid - nb);
    small_gemm_body<MT, 4>(hh, (bid - nb - nm) % gxh, (bid - nb - nm) / gxh);
}

// =================================================================================================
// The text attention in FOLDED form (inference only: nothing here is taped for a backward).
// model.py:129-141 per decode step: t = W_in h1, s_l = ctx_l . t, alpha = softmax(s), wc = sum alpha_l ctx_l,
// h~ = tanh(W_out [wc ; h1]).  The context does not change during an episode, so two products leave the per-step
// chain for good (sf_text_fold_build, once per episode):
//     ctx_q = ctx W_in           s_l = ctx_q[l] . h1                     (no t = W_in h1 product per step)
//     ctx_o = ctx W_out[:, :H]^T W_out [wc ; h1] = sum alpha_l ctx_o[l] + W_out[:, H:] h1
// A step then needs, behind the cell: this body (scores + softmax + z = sum alpha_l ctx_o[l]) BESIDE the product
// y = W_out[:, H:] h1 in one launch, and h~ = tanh(z + y) is formed by the A-prologue of the next product
// (t_a = W_h h~ + b: sf_gemm_small.h, APRO) -- two dependent launches fewer per decode step.
// The body reads TWO context tensors, so a sample is split over TXF_G = 4 workgroups (positions [g Lg, (g + 1) Lg)): a
// CU sustains ~25-45 GB/s of loads and bytes per workgroup are what the stage costs.  Each keeps a flash-style piece
// (m, l, unnormalised z); the last arriver of a sample merges them in the same launch (measured, round 6: two groups
// merged by the consumer's prologue: stage 10.3 us + consumer 9.4 us; four groups merged here: 10.9 + 7.4).
// =================================================================================================

struct TxtFoldArgs {
    const float* ctx_q;    // [B, L, H]
    const float* ctx_o;    // [B, L, H]
    const uint8_t* mask;   // [B, L] (1 = padding) or null
    int L, H;
    const float* vec;      // h1 as the text attention sees it (eval: h1 itself) [B, ldvec]
    int ldvec;
    float* part;           // [B][G][H + 64], G <= TXF_G: z | e[l - g Lg] (<= 62) | m at H + 62 | l at H + 63
    unsigned* counter;     // [B] monotonic tickets (zero before the first launch; every launch adds TXF_G per sample)
    float* z;              // out [B, ldz]: sum_l alpha_l ctx_o[l] (merged, normalised)
    int ldz;
    float* alpha;          // out [B, L]: the attention weights (the tape's contract), or null
};

// One group's share -- positions [g LG, (g + 1) LG) of sample b: scores, local softmax piece (m, l, e), unnormalised
// z = sum e_l ctx_o[l] -- published WRITE-THROUGH like the split visual attention's partials (visual_split_body<0>:
// sc1 stores, drain, agent-scope ticket; no cache-wide fence), and the workgroup that draws the sample's LAST ticket
// merges the G pieces (sc1 loads) into z [H] and alpha [L]: no spinning, no extra launch.
// G is the group count of the launch: TXF_G everywhere but in launch (1) of the projected chain at a batch whose
// four-group grid does not fit the device at once (proj_text_groups_plan).  The tickets stay aligned whatever launches
// share a workspace: a block adds TXF_G / G, so EVERY launch adds TXF_G per sample and the last arriver is the one that
// reads TXF_G - TXF_G / G in the low bits.  The records are [B][G][H + 64] in a scratch sized for TXF_G.
template <int RPW, int G>
__device__ __forceinline__ void text_fold_body(const TxtFoldArgs& a, int g, int b) {
    constexpr int NW = SMALL_WAVES, SL = 4, LG = NW * RPW;
    static_assert(LG <= 62, "a group's weights live in 62 record slots");
    static_assert(G >= 1 && G <= TXF_G && TXF_G % G == 0, "a launch adds TXF_G tickets per sample; the scratch holds TXF_G");
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    __shared__ float4 slots[SL][TXT_CPL * 64];
    __shared__ float s_score[LG];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, H = a.H, n4 = H >> 2;
    const int pstride = H + 64;
    const float4* cq = reinterpret_cast<const float4*>(a.ctx_q) + (size_t)b * L * n4;
    const float4* co = reinterpret_cast<const float4*>(a.ctx_o) + (size_t)b * L * n4;
    const bool use_mask = a.mask != nullptr;
    const uint8_t* mrow = use_mask ? a.mask + (size_t)b * L : reinterpret_cast<const uint8_t*>(cq);
    // a group whose positions are ALL padding (short instructions: the length-sorted minibatch ends far below L)
    // pulls nothing: its piece is (m = -inf, l = 0, z = 0) and it only draws its ticket
    const int lt = g * LG + tid;
    const bool padded = tid >= LG || lt >= L || (use_mask && mrow[min(lt, L - 1)] != 0);
    const bool empty = __syncthreads_and(padded) != 0;              // block-uniform
    float m = -INFINITY, e = 0.f, lsum = 0.f;
    float4 p[TXT_CPL];
#pragma unroll
    for (int i = 0; i < TXT_CPL; ++i) p[i] = f4zero();
    if (!empty) {
    // straight-line loads, clamped indices, value selects (sf_rows.h): every row of both tensors is in flight at once
    float4 xq[RPW][TXT_CPL], xo[RPW][TXT_CPL];
    uint8_t mk[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int l = g * LG + wave * RPW + r;
        const int lc = min(l, L - 1);
#pragma unroll
        for (int i = 0; i < TXT_CPL; ++i) {
            const int c = lane + 64 * i;
            const float4 tq = cq[(size_t)lc * n4 + min(c, n4 - 1)];
            const float4 to = co[(size_t)lc * n4 + min(c, n4 - 1)];
            const bool ok = l < L && c < n4;
            xq[r][i] = ok ? tq : f4zero();
            xo[r][i] = ok ? to : f4zero();
        }
        mk[r] = mrow[lc];
    }
    float4 v[TXT_CPL];
#pragma unroll
    for (int i = 0; i < TXT_CPL; ++i) {
        const int c = lane + 64 * i;
        const float4 t = reinterpret_cast<const float4*>(a.vec + (size_t)b * a.ldvec)[min(c, n4 - 1)];
        v[i] = c < n4 ? t : f4zero();
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < TXT_CPL; ++i) d += dot4(xq[r][i], v[i]);
        d = wave_sum(d);
        const int l = g * LG + wave * RPW + r;
        if (lane == 0) s_score[wave * RPW + r] = (l >= L || (use_mask && mk[r])) ? -INFINITY : d;
    }
    __syncthreads();
    const float sc = lane < LG ? s_score[lane] : -INFINITY;
    m = wave_max(sc);                                              // -inf: every position of this group is padding
    e = sc > -INFINITY ? expf(sc - m) : 0.f;
    lsum = wave_sum(e);
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const float er = __shfl(e, wave * RPW + r, WAVE);
#pragma unroll
        for (int i = 0; i < TXT_CPL; ++i) f4fma(p[i], er, xo[r][i]);
    }
    }   // !empty
    float* r0 = a.part + (size_t)b * G * pstride;
    float* rec = r0 + (size_t)g * pstride;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(rec, 0, pstride * 4, 0x00020000);
    block_row_sum<TXT_CPL, NW, SL>(p, slots, n4, [&](int c, float4 t) {
        const v4u w{__float_as_uint(t.x), __float_as_uint(t.y), __float_as_uint(t.z), __float_as_uint(t.w)};
        __builtin_amdgcn_raw_buffer_store_b128(w, rs, c * 16, 0, 16);
    });
    if (wave == 0) {
        if (lane < LG) __hip_atomic_store(rec + H + lane, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) {
            __hip_atomic_store(rec + H + 62, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(rec + H + 63, lsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // EVERY storing wave drains
    __syncthreads();
    if (tid == 0)
        s_last = (__hip_atomic_fetch_add(a.counter + b, (unsigned)(TXF_G / G), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &
                  (unsigned)(TXF_G - 1)) == (unsigned)(TXF_G - TXF_G / G);
    __syncthreads();
    if (!s_last) return;

    // ---- the sample's last arriver merges the pieces
    auto ldf = [&](float* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    float mg[G], kk[G];
    float M = -INFINITY;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        mg[k] = ldf(r0 + (size_t)k * pstride + H + 62);
        M = fmaxf(M, mg[k]);
    }
    float Lsum = 0.f;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        kk[k] = mg[k] > -INFINITY ? expf(mg[k] - M) : 0.f;      // an empty group: weight 0 (its l is 0 too)
        Lsum = fmaf(ldf(r0 + (size_t)k * pstride + H + 63), kk[k], Lsum);
    }
    const float inv = 1.0f / Lsum;                              // (a sample always has an unmasked position)
#pragma unroll
    for (int k = 0; k < G; ++k) kk[k] *= inv;
    if (a.alpha) {
        for (int l = tid; l < L; l += NW * 64) {
            const int gk = l / LG;
            float w = kk[0];
#pragma unroll
            for (int k = 1; k < G; ++k) w = gk == k ? kk[k] : w;
            a.alpha[(size_t)b * L + l] = ldf(r0 + (size_t)gk * pstride + H + (l - gk * LG)) * w;
        }
    }
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(r0, 0, G * pstride * 4, 0x00020000);
    float4* zrow = reinterpret_cast<float4*>(a.z + (size_t)b * a.ldz);
    for (int c = tid; c < n4; c += NW * 64) {
        float4 t = f4zero();
#pragma unroll
        for (int k = 0; k < G; ++k) {
            const v4u pk = __builtin_amdgcn_raw_buffer_load_b128(rs0, k * pstride * 4 + c * 16, 0, 16);
            t.x = fmaf(kk[k], __uint_as_float(pk.x), t.x);
            t.y = fmaf(kk[k], __uint_as_float(pk.y), t.y);
            t.z = fmaf(kk[k], __uint_as_float(pk.z), t.z);
            t.w = fmaf(kk[k], __uint_as_float(pk.w), t.w);
        }
        zrow[c] = t;
    }
}

// the folded text stage: [text_fold groups | y = W_out[:, H:] h1 | t_v' = W_h h1 + b] in ONE grid
template <int RPW>
__global__ __launch_bounds__(SMALL_WAVES * 64) void pair_textfold_small_small_kernel(TxtFoldArgs t, int nt, SmallArgs a,
                                                                                    int gxa, int na, SmallArgs b, int gxb) {
    const int bid = blockIdx.x;
    if (bid < nt)
        text_fold_body<RPW, TXF_G>(t, bid % TXF_G, bid / TXF_G);
    else if (bid < nt + na)
        small_gemm_body<1, 4>(a, (bid - nt) % gxa, (bid - nt) / gxa);
    else
        small_gemm_body<1, 4>(b, (bid - nt - na) % gxb, (bid - nt - na) / gxb);
}

// launch (1) of the projected chain: [projected attention partials of step t + 1 | text_fold groups | y = W_out[:, H:] h1]
// (the partials blocks pull the most bytes: first in the grid; proj_partials_body keeps the kernel within 128 registers,
// two workgroups per CU).  VIS false: the instantiation without the partials body (nv == 0: an episode's last step, or
// the partials ride in launch (2)) -- the text groups alone need far fewer registers and run three or more to a CU.
// G: text groups per sample (proj_text_groups_plan; last, so that the profile name still reads <RPW, true, ...>).
template <int RPW, bool VIS, int G = TXF_G>
__global__ __launch_bounds__(SMALL_WAVES * 64) void pair_proj_textfold_kernel(VisArgs v, VisSplit sp, int nv, TxtFoldArgs t, int nt,
                                                                            SmallArgs a, int gxa) {
    const int bid = blockIdx.x;
    if (VIS && bid < nv) {
        proj_partials_body(v, sp, bid % PPB_G, bid / PPB_G);
    } else if (bid < nv + nt) {
        text_fold_body<RPW, G>(t, (bid - nv) % G, (bid - nv) / G);
    } else {
        small_gemm_body<1, 4>(a, (bid - nv - nt) % gxa, (bid - nv - nt) / gxa);
    }
}

// t_a = W_h tanh(z + y) + b (A-prologue: z = the merged attention sum of the text_fold launch) beside q' = W_v^T t_v'
template <int MTB>
__global__ __launch_bounds__(SMALL_WAVES * 64) void pair_apro_small_kernel(SmallArgs a, int gxa, int na, SmallArgs b, int gxb) {
    const int bid = blockIdx.x;
    if (bid < na)
        small_gemm_body<1, 4, false, true>(a, bid % gxa, bid / gxa);
    else
        small_gemm_body<MTB, 2>(b, (bid - na) % gxb, (bid - na) / gxb);
}

// Deferred gradient of the instruction context (model.py:129-139 backward, summed over an episode):
// dctx[b,l,:] += sum_t ( alpha[t,b,l] dwc[t,b,:] + ds[t,b,l] tt[t,b,:] ).  The per-step form reads and
// writes the whole [B,L,H] gradient S times (2 x 16 MB per step at the headline shape); this reads each
// step's two H-vectors once.  One block per sample; thread = one float4 column x every 8th row.

__global__ __launch_bounds__(1024) void ctx_grad_kernel(const float* alpha, const float* ds,
                                                        const float* dcat2, int lddc, const float* tt,
                                                        int S, int B, int L, int H, float* dctx) {
    extern __shared__ float s_w[];                       // [S][2][L]: alpha, ds of this sample
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < S * L; i += 1024) {
        const int t = i / L, l = i - t * L;
        s_w[(t * 2 + 0) * L + l] = alpha[((size_t)t * B + b) * L + l];
        s_w[(t * 2 + 1) * L + l] = ds[((size_t)t * B + b) * L + l];
    }
    __syncthreads();
    const int n4 = H >> 2;
    const int c = tid % n4, lg = tid / n4;               // n4 = 128: 8 row groups
    const int ngroups = 1024 / n4;
    if (lg >= ngroups) return;
    float4 acc[CG_ROWS];
#pragma unroll
    for (int r = 0; r < CG_ROWS; ++r) acc[r] = f4zero();
    for (int t = 0; t < S; ++t) {
        const float4 d = reinterpret_cast<const float4*>(dcat2 + ((size_t)t * B + b) * lddc)[c];
        const float4 x = reinterpret_cast<const float4*>(tt + ((size_t)t * B + b) * H)[c];
#pragma unroll
        for (int r = 0; r < CG_ROWS; ++r) {
            const int l = lg + ngroups * r;
            if (l < L) {
                f4fma(acc[r], s_w[(t * 2 + 0) * L + l], d);
                f4fma(acc[r], s_w[(t * 2 + 1) * L + l], x);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < CG_ROWS; ++r) {
        const int l = lg + ngroups * r;
        if (l < L) {
            float4* o = reinterpret_cast<float4*>(dctx + ((size_t)b * L + l) * H) + c;
            float4 v = *o;
            f4add(v, acc[r]);
            *o = v;
        }
    }
}


// Backward: the visual-attention backward of a step (needs the input gradient of the LSTM) beside the
// recurrent data gradient dh0 = dgates W_hh (needs only dgates): independent, one launch.
// Blocks [0, nv): attention backward (12 waves); the rest: the small product (threads >= 512 leave).
template <int MT, int CPW, bool H16 = false>
__global__ __launch_bounds__(VIS_NW * 64) void pair_visbwd_small_kernel(VisArgs v, int nv, SmallArgs b,
                                                                       int gxb) {
    const int bid = blockIdx.x;
    if (bid < nv) {
        visual_attn_body<1, H16>(v, bid);
    } else {
        if (threadIdx.x >= SMALL_WAVES * 64) return;
        small_gemm_body<MT, CPW>(b, (bid - nv) % gxb, (bid - nv) / gxb);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// LAUNCHERS.  Each one gates on the named rules of sf_attention_plan.h (pure host code, tests/test_attention_plan_host.py)
// -- their ORDER decides between SF_ERR_UNSUPPORTED and SF_ERR_ARG --, fills the kernels' argument structs, turns a
// ladder's value into a template argument with with_index, and launches.
// Storage dispatch.  EVERY launcher below that takes a PanoSrc / CandSrc launches through one of these two macros (or
// returns before launching), so a table registered as binary16 can only reach an instantiation that reads 8-byte chunks:
// an fp32 read of it would run off the end of the table.  A half source in dense form is a caller's error.  The
// binary16 instantiation is K<..., true>, or K<true> under the name "<f16>".
// ------------------------------------------------------------------------------------------------
#define SF_LAUNCH_INST_H16(half, K, targs, ...)                             \
    do {                                                                    \
        if (half) SF_LAUNCH_INST(K, (SF_TARGS targs, true), __VA_ARGS__);   \
        else SF_LAUNCH_INST(K, targs, __VA_ARGS__);                         \
    } while (0)
#define SF_LAUNCH_H16_AS(half, name, K, ...)                         \
    do {                                                             \
        if (half) SF_LAUNCH_AS(name "<f16>", K<true>, __VA_ARGS__);  \
        else SF_LAUNCH_AS(name, K<false>, __VA_ARGS__);              \
    } while (0)
template <typename Src>
static inline bool half_misuse(const Src& s) { return s.half && s.dense; }
static inline RowShape shape(const PanoSrc& s) { return RowShape{s.V, s.IMG, s.LOC, s.dense != nullptr, s.half != 0}; }
static inline RowShape shape(const CandSrc& s) { return RowShape{s.A, s.IMG, s.LOC, s.dense != nullptr, s.half != 0}; }
// known: with_index found the instantiation (the gate before it accepts nothing else)
static inline int launched(bool known) { return known ? launch_status() : SF_ERR_UNSUPPORTED; }

bool visual_attn_f64_supported(const PanoSrc& src, int B) { return split_rows_fit(shape(src), B); }

int visual_attn(int mode, const PanoSrc& src, int B, const float* vec, int ldvec, float* alpha,
                float* out, int ldo, const Dropout& drop, int drop_col0, hipStream_t st,
                float* split_part, unsigned* split_counter, const double* vec64, int vec_slabs, long vec_slab_stride) {
    if (!pano_rows_fit(shape(src)) || !aligned4(ldvec, ldo)) return SF_ERR_UNSUPPORTED;
    if (half_misuse(src)) return SF_ERR_ARG;
    VisArgs a{src, vec, ldvec, alpha, out, ldo, drop, drop_col0, vec64, mode == 1 ? vec_slabs : 0, vec_slab_stride};
    if (mode != 1 && vec_slabs > 1) return SF_ERR_UNSUPPORTED;
    // small batches: VSP_G workgroups per sample (see visual_attn_split_kernel)
    const bool split = mode == 0 && split_part && split_counter && in_split_range(src.V, B);
    if (vec64 && !split) return SF_ERR_UNSUPPORTED;   // float64 scores: the split forward only (visual_attn_f64_supported)
    if (vec64)
        SF_LAUNCH_H16_AS(src.half, "visual_attn_split_f64_kernel", visual_attn_split_f64_kernel, dim3(VSP_G, B),
                         dim3(VSP_NW * 64), 0, st, a, VisSplit{split_part, split_counter, nullptr});
    else if (split)
        SF_LAUNCH_H16_AS(src.half, "visual_attn_split_kernel", visual_attn_split_kernel, dim3(VSP_G, B),
                         dim3(VSP_NW * 64), 0, st, a, VisSplit{split_part, split_counter, nullptr});
    else if (mode == 0)
        SF_LAUNCH_INST_H16(src.half, visual_attn_kernel, (0), dim3(B), dim3(VIS_NW * 64), 0, st, a);
    else
        SF_LAUNCH_INST_H16(src.half, visual_attn_kernel, (1), dim3(B), dim3(VIS_NW * 64), 0, st, a);
    return launch_status();
}

template <int MODE>
static int text_attn_launch(const TxtArgs& a, int B, hipStream_t st) {
    return launched(with_index(text_rpw(a.L), [&](auto r) {
        constexpr int R = decltype(r)::value;                   // (the profile has always said "MODE" for the second one)
        SF_LAUNCH_AS((inst_name<text_attn_kernel<R, MODE>, R>("text_attn_kernel", ", MODE")), (text_attn_kernel<R, MODE>),
                     dim3(B), dim3(TXT_NW * 64), 0, st, a);
    }, ints<1, 5, 8>{}));
}

int text_attn_fwd(const float* ctx, const uint8_t* mask, int B, int L, int H, const float* t,
                  int ldt, float* alpha, float* wc, int ldwc, hipStream_t st,
                  const int32_t* ctx_row) {
    if (!text_rows_fit(L, TXT_MAX_L, H, ldt | ldwc)) return SF_ERR_UNSUPPORTED;
    TxtArgs a{ctx, mask, L, H, t, ldt, nullptr, 0, alpha, wc, ldwc, nullptr, ctx_row, nullptr};
    return text_attn_launch<0>(a, B, st);
}

int text_attn_bwd(const float* ctx, int B, int L, int H, const float* dwc, int lddwc,
                  const float* t, int ldt, const float* alpha, float* dt, int lddt, float* dctx,
                  hipStream_t st, float* ds_out, const int32_t* ctx_row) {
    if (!text_rows_fit(L, TXT_MAX_L, H, ldt | lddwc | lddt) || (ctx_row && dctx)) return SF_ERR_UNSUPPORTED;
    TxtArgs a{ctx, nullptr, L, H, dwc, lddwc, t, ldt, const_cast<float*>(alpha), dt, lddt, dctx, ctx_row, ds_out};
    return text_attn_launch<1>(a, B, st);
}

int ctx_grad_accum(const float* alpha, const float* ds, const float* dcat2, int lddc, const float* tt,
                   int S, int B, int L, int H, float* dctx, hipStream_t st) {
    if (!ctx_grad_supported(S, L, H) || !aligned4(lddc)) return SF_ERR_UNSUPPORTED;
    SF_LAUNCH(ctx_grad_kernel, dim3(B), dim3(1024), (size_t)S * 2 * L * sizeof(float), st, alpha,
                       ds, dcat2, lddc, tt, S, B, L, H, dctx);
    return launch_status();
}

int score_fwd(const CandSrc& src, int B, int D, const float* r, const float* wt, const float* b_a,
              const float* b_out, float* logit, hipStream_t st) {
    if (!cand_rows_fit(shape(src))) return SF_ERR_UNSUPPORTED;
    if (half_misuse(src)) return SF_ERR_ARG;
    ScoreArgs a{src, src.IMG + src.LOC, nullptr, r, wt, b_a, b_out, D, logit, nullptr, nullptr, CeSrc{}};
    SF_LAUNCH_H16_AS(src.half, "score_fwd_kernel", score_fwd_kernel, dim3(B), dim3(SC_NW * 64), 0, st, a);
    return launch_status();
}

int score_glue_fwd(const CandSrc& src, int B, int D, const float* r, const float* wt,
                   const float* b_a, const float* b_out, const FGlue& g, hipStream_t st) {
    if (!cand_rows_fit(shape(src))) return SF_ERR_UNSUPPORTED;
    if (half_misuse(src)) return SF_ERR_ARG;
    ScoreArgs a{src, src.IMG + src.LOC, nullptr, r, wt, b_a, b_out, D, g.logit, nullptr, nullptr, CeSrc{}};
    SF_LAUNCH_H16_AS(src.half, "score_glue_kernel", score_glue_kernel, dim3(B), dim3(SC_NW * 64), 0, st, a, g);
    return launch_status();
}

// score_glue_fwd beside the phase-2 merge of visual-attention partials written by an earlier phase-1 launch
int pair_score_merge(const CandSrc& src, int B, int D, const float* r, const float* wt, const float* b_a,
                     const float* b_out, const FGlue& g, const PanoSrc& psrc, float* alpha, float* out, int ldo,
                     const Dropout& drop, int drop_col0, float* split_part, hipStream_t st) {
    if (!cand_rows_fit(shape(src))) return SF_ERR_UNSUPPORTED;
    if (!split_part || !in_split_range(psrc.V, B) || !aligned4(ldo)) return SF_ERR_UNSUPPORTED;
    if (half_misuse(src) || half_misuse(psrc)) return SF_ERR_ARG;
    ScoreArgs a{src, src.IMG + src.LOC, nullptr, r, wt, b_a, b_out, D, g.logit, nullptr, nullptr, CeSrc{}};
    VisArgs va{psrc, nullptr, 0, alpha, out, ldo, drop, drop_col0};
    const VisSplit sp{split_part, nullptr, g_trace};
    SF_LAUNCH_H16_AS(src.half, "pair_score_merge_kernel", pair_score_merge_kernel, dim3(2 * B), dim3(SC_NW * 64), 0, st, a,
                     g, B, va, sp);
    return launch_status();
}

int score_bwd(const CandSrc& src, int B, const float* dlogit, float* dr, float* dc,
              hipStream_t st, const CeSrc* ce) {
    if (!cand_rows_fit(shape(src))) return SF_ERR_UNSUPPORTED;
    ScoreArgs a{src, src.IMG + src.LOC, nullptr, nullptr, nullptr, nullptr, nullptr, 0, const_cast<float*>(dlogit), dr, dc,
                ce ? *ce : CeSrc{}};
    if ((ce && ce->ld < src.A) || half_misuse(src)) return SF_ERR_ARG;
    SF_LAUNCH_H16_AS(src.half, "score_bwd_kernel", score_bwd_kernel, dim3(B), dim3(SC_NW * 64), 0, st, a);
    return launch_status();
}

// ---- paired launches (host side).  SF_ERR_UNSUPPORTED = "not pairable": the caller launches the
// two kernels one after the other instead.  What each accepts of a small product: pair_*_accepts, which the chains of
// sf_api_follower.hip ask as well.
int pair_small_small(const SmallPlan& a, const SmallPlan& b, hipStream_t st) {
    if (!pair_small_small_accepts(a.inst(), b.inst())) return SF_ERR_UNSUPPORTED;
    const int na = a.gx * a.gy, nb = b.gx * b.gy;
    const dim3 grid(na + nb), block(SMALL_WAVES * 64);
    return launched(with_index(b.mt, [&](auto m) {
        SF_LAUNCH_INST(pair_small_small_kernel, (1, 4, decltype(m)::value, 4), grid, block, 0, st, a.args, a.gx, na, b.args, b.gx);
    }, ints<1, 2, 4>{}));
}

// The folded text stage of an inference decode step (see text_fold_body): SF_ERR_UNSUPPORTED = shapes outside the
// instantiations (the caller runs the unfolded stages).
int pair_textfold_small_small(const float* ctx_q, const float* ctx_o, const uint8_t* mask, int B, int L, int H,
                              const float* vec, int ldvec, float* part, unsigned* counter, float* z, int ldz, float* alpha,
                              const SmallPlan& a, const SmallPlan& b, hipStream_t st) {
    if (!pair_textfold_small_small_accepts(a.inst(), b.inst())) return SF_ERR_UNSUPPORTED;
    if (!text_fold_fits(B, L, H, ldvec, ldz) || !counter || !z) return SF_ERR_UNSUPPORTED;
    const TxtFoldArgs ta{ctx_q, ctx_o, mask, L, H, vec, ldvec, part, counter, z, ldz, alpha};
    const int nt = TXF_G * B, na = a.gx * a.gy, nb = b.gx * b.gy;
    const dim3 grid(nt + na + nb), block(SMALL_WAVES * 64);
    return launched(with_index(fold_rpw(L, TXF_G), [&](auto r) {
        constexpr int R = decltype(r)::value;
        SF_LAUNCH_INST(pair_textfold_small_small_kernel, (R), grid, block, 0, st, ta, nt, a.args, a.gx, na, b.args, b.gx);
    }, ints<1, 2, 3, 5>{}));
}

// a: the product whose A operand the prologue forms (a.args.apro_part set by the caller), b: a plain small product
int pair_apro_small(const SmallPlan& a, const SmallPlan& b, hipStream_t st) {
    if (!pair_apro_small_accepts(a.inst(), b.inst()) || !a.args.apro_part || a.args.sg.total != a.args.sg.n0)
        return SF_ERR_UNSUPPORTED;
    const int na = a.gx * a.gy, nb = b.gx * b.gy;
    const dim3 grid(na + nb), block(SMALL_WAVES * 64);
    return launched(with_index(b.mt, [&](auto m) {
        SF_LAUNCH_INST(pair_apro_small_kernel, (decltype(m)::value), grid, block, 0, st, a.args, a.gx, na, b.args, b.gx);
    }, ints<1, 2, 4>{}));
}

int pair_small_text(const SmallPlan& a, const float* ctx, const uint8_t* mask, int B, int L, int H,
                    const float* t, int ldt, float* alpha, float* wc, int ldwc,
                    const int32_t* ctx_row, hipStream_t st) {
    if (!pair_small_text_accepts(a.inst())) return SF_ERR_UNSUPPORTED;
    if (!text_rows_fit(L, TXT_MAX_L, H, ldt | ldwc)) return SF_ERR_UNSUPPORTED;
    TxtArgs ta{ctx, mask, L, H, t, ldt, nullptr, 0, alpha, wc, ldwc, nullptr, ctx_row, nullptr};
    const int na = a.gx * a.gy;
    const dim3 grid(na + B), block(TXT_NW * 64);
    return launched(with_index(text_rpw(L), [&](auto r) {
        SF_LAUNCH_INST(pair_small_text_kernel, (4, 2, decltype(r)::value), grid, block, 0, st, a.args, a.gx, na, ta);
    }, ints<1, 5, 8>{}));
}

// visual-attention backward (mode 1 of visual_attn) paired with a small product (mt 1, cpw 16: the
// K = 4H recurrent data gradient); SF_ERR_UNSUPPORTED = not pairable, launch separately
int pair_visbwd_small(const PanoSrc& src, int B, const float* vec, int ldvec, float* alpha, float* out,
                      int ldo, const Dropout& drop, int drop_col0, const SmallPlan& b, hipStream_t st, int vec_slabs,
                      long vec_slab_stride) {
    if (!pair_visbwd_small_accepts(b.inst())) return SF_ERR_UNSUPPORTED;
    if (!pano_rows_fit(shape(src)) || !aligned4(ldvec, ldo)) return SF_ERR_UNSUPPORTED;
    if (half_misuse(src)) return SF_ERR_ARG;
    VisArgs va{src, vec, ldvec, alpha, out, ldo, drop, drop_col0, nullptr, vec_slabs, vec_slab_stride};
    const int nb = b.gx * b.gy;
    SF_LAUNCH_INST_H16(src.half, pair_visbwd_small_kernel, (1, 16), dim3(B + nb), dim3(VIS_NW * 64), 0, st, va, B, b.args, b.gx);
    return launch_status();
}

// ---- the projected decode chain (sf_api_follower.hip: tail_proj).  proj_chain_supported is the PLAN: both launchers below check
// it again and return SF_ERR_UNSUPPORTED before launching, but tail_proj asks first so that it declines as a whole.
// Here: what the rule of sf_attention_plan.h cannot see -- the tables are there, candidates and panorama share one.
bool proj_chain_supported(const CandSrc& us, const PanoSrc* xn, int B, int H, int L, const ProjTables& pt) {
    if (!pt.pv || !pt.pa || !pt.lv || !pt.la || !us.table || !us.a_num) return false;
    if (xn && (xn->table != us.table || xn->V != us.V)) return false;
    const RowShape x = xn ? shape(*xn) : RowShape{};
    return proj_chain_supported(shape(us), xn ? &x : nullptr, B, H, L, pt.H, pt.ld);
}

static VisArgs proj_vis_args(const PanoSrc& xn, const ProjTables& pt, const float* h1, int ldh1, float* alpha, float* out,
                             int ldo, const Dropout& drop, int drop_col0) {
    VisArgs va{xn, h1, ldh1, alpha, out, ldo, drop, drop_col0};
    va.pv = pt.pv; va.lv = pt.lv; va.ldp = pt.ld; va.pH = pt.H;
    return va;
}

// step 0's head: the visual attention straight from h through PV / LV, one launch (no t_v', no q)
int visual_attn_proj(const CandSrc& us, const PanoSrc& x, int B, int H, int L, const ProjTables& pt, const float* h, int ldh,
                     float* alpha, float* out, int ldo, const Dropout& drop, int drop_col0, float* split_part,
                     unsigned* counter, hipStream_t st) {
    if (!proj_chain_supported(us, &x, B, H, L, pt) || !aligned4(ldh, ldo) || !split_part || !counter) return SF_ERR_UNSUPPORTED;
    const VisArgs va = proj_vis_args(x, pt, h, ldh, alpha, out, ldo, drop, drop_col0);
    SF_LAUNCH(visual_attn_split_proj_kernel, dim3(VSP_G, B), dim3(VSP_NW * 64), 0, st, va, VisSplit{split_part, counter, nullptr});
    return launch_status();
}

// ---- text groups per sample of launch (1): proj_text_groups_plan (sf_attention_plan.h) decides from the resident
// workgroups of the four-group launch (1) with partials on the current device: CUs x what the runtime's occupancy query
// gives pair_proj_textfold_kernel<R, true, TXF_G> (R: the four-group ladder's rung for L, text_rung).  Asked once per
// device and kept (sf_projected_build asks ahead of any capture: proj_text_slots_warm); 0 = unknown, four groups.
int g_proj_text_groups = 0;
static_assert(TXF_G == 4, "pair_proj_textfold names its instantiations <R, true, 2> and <R, true, 4>");
static int proj_text_slots(int rung) {
    constexpr int kMaxDev = 64;
    static std::atomic<int> cache[kMaxDev][4];                   // slots + 1 (0: not asked yet)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) {
        (void)hipGetLastError();
        return 0;
    }
    if (cache[dev][0].load(std::memory_order_acquire) == 0) {
        int cus = 0, per[4] = {0, 0, 0, 0};
        bool ok = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess;
#define SF_OCC(i, R)                                                                                               \
    ok = ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per[i], pair_proj_textfold_kernel<R, true, TXF_G>,   \
                                                            SMALL_WAVES * 64, 0) == hipSuccess
        SF_OCC(0, 1); SF_OCC(1, 2); SF_OCC(2, 3); SF_OCC(3, 5);
#undef SF_OCC
        if (!ok) (void)hipGetLastError();
        for (int r = 3; r >= 0; --r)                                 // (rung 0 last: it is the "asked" mark read above)
            cache[dev][r].store((ok && cus > 0 && per[r] > 0 ? cus * per[r] : 0) + 1, std::memory_order_release);
    }
    return cache[dev][rung].load(std::memory_order_acquire) - 1;
}
void proj_text_slots_warm() { (void)proj_text_slots(0); }

// launch (1): folded text attention (+ its in-launch merge)  ||  y  ||  projected partials of step t + 1 (`xn` null: none)
int pair_proj_textfold(const float* ctx_q, const float* ctx_o, const uint8_t* mask, int B, int L, int H, const float* vec,
                       int ldvec, float* part, unsigned* counter, float* z, int ldz, float* alpha, const SmallPlan& y,
                       const CandSrc& us, const PanoSrc* xn, const ProjTables& pt, const float* h1, int ldh1, float* split_part,
                       hipStream_t st, const float* gf) {
    if (!pair_proj_textfold_accepts(y.inst()) || !proj_chain_supported(us, xn, B, H, L, pt)) return SF_ERR_UNSUPPORTED;
    if (!aligned4(ldvec, ldh1, ldz) || !counter || !z || ldz < H || (xn && !split_part)) return SF_ERR_UNSUPPORTED;
    if (xn && !proj_partials_supported(xn->IMG, xn->LOC)) return SF_ERR_UNSUPPORTED;
    if (gf && (!xn || !proj_partials_supported(4 * H, xn->LOC))) return SF_ERR_UNSUPPORTED;
    const TxtFoldArgs ta{ctx_q, ctx_o, mask, L, H, vec, ldvec, part, counter, z, ldz, alpha};
    VisArgs va = xn ? proj_vis_args(*xn, pt, h1, ldh1, nullptr, nullptr, 0, Dropout{}, 0) : VisArgs{};
    if (gf) {             // the row source in gate space: row (vp, v) of gf, 4H floats, in the slots of the image row
        va.src.table = gf;
        va.src.IMG = 4 * H;
    }
    const VisSplit sp{split_part, nullptr, g_trace};
    const int nv = xn ? PPB_G * B : 0, na = y.gx * y.gy;
    const int force = g_proj_text_groups;
    // (the slots are asked for only where the rule can say two: no runtime query on a path that never takes them)
    const int slots = xn && L <= TXF_G2_MAX_L && force == 0 ? proj_text_slots(text_rung(L, TXF_G)) : 0;
    int blocks = 0;
    const int G = proj_text_groups_plan(B, L, xn != nullptr, na, slots, force, &blocks);
    const int nt = G * B;
    const dim3 grid(blocks), block(SMALL_WAVES * 64);
    return launched(with_index(fold_rpw(L, G), [&](auto r) {
        constexpr int R = decltype(r)::value;
        if (nv && G == 2) SF_LAUNCH_INST(pair_proj_textfold_kernel, (R, true, 2), grid, block, 0, st, va, sp, nv, ta, nt, y.args, y.gx);
        else if (nv) SF_LAUNCH_INST(pair_proj_textfold_kernel, (R, true, 4), grid, block, 0, st, va, sp, nv, ta, nt, y.args, y.gx);
        else SF_LAUNCH_INST(pair_proj_textfold_kernel, (R, false), grid, block, 0, st, va, sp, nv, ta, nt, y.args, y.gx);
    }, ints<1, 2, 3, 5>{}));
}

// launch (2): scoring + glue on projected candidate rows  ||  vphase 2: merge of launch (1)'s partials; 0: the whole
// projected attention of step t + 1 (needs `counter`); `xn` null: the scoring alone
int pair_proj_score(const CandSrc& us, int B, int H, int L, const ProjTables& pt, const float* z, int ldz, const float* y, int ldy,
                    const FGlue& g, const PanoSrc* xn, int vphase, const float* h1, int ldh1, float* alpha, float* out, int ldo,
                    const Dropout& drop, int drop_col0, float* split_part, unsigned* counter, hipStream_t st,
                    const GateRows* gate, const SmallPlan* hh) {
    if (!proj_chain_supported(us, xn, B, H, L, pt) || !aligned4(ldz, ldy, ldh1)) return SF_ERR_UNSUPPORTED;
    if (hh && (!xn || vphase != 2 || !gate || !gate->xg_f || !gate->xg_h || hh->args.y != gate->xg_h ||
               !pair_proj_score_hh_accepts(hh->inst())))
        return SF_ERR_UNSUPPORTED;
    if (xn && (!split_part || !aligned4(ldo) || (vphase != 0 && vphase != 2) || (vphase == 0 && !counter))) return SF_ERR_UNSUPPORTED;
    if (gate && (!gate->gu || !gate->gl || !gate->xg_next)) return SF_ERR_UNSUPPORTED;
    ProjScoreArgs a{us, pt.pa, pt.la, pt.ld, H, z, y, ldz, ldy};
    if (gate) { a.gu = gate->gu; a.gl = gate->gl; a.xg_next = gate->xg_next; }
    VisArgs va = xn ? proj_vis_args(*xn, pt, h1, ldh1, alpha, out, ldo, drop, drop_col0) : VisArgs{};
    if (gate && gate->xg_f) {
        // launch (1) summed gate-space rows: records of 4H + LOC floats; the 4H part to xg_f, the LOC part to its columns
        // of `out`
        if (!xn || vphase != 2 || drop.on() || !gate->gf || !proj_partials_supported(4 * H, xn->LOC)) return SF_ERR_UNSUPPORTED;
        va.out = out + xn->IMG;
        va.src.table = gate->gf;
        va.src.IMG = 4 * H;
        va.out_img = gate->xg_f;
        va.ld_img = 4 * H;
    }
    const VisSplit sp{split_part, counter, g_trace};
    const dim3 block(SMALL_WAVES * 64);
    if (hh) {
        const int nh = hh->gx * hh->gy;
        return launched(with_index(hh->mt, [&](auto m) {
            constexpr int MT = decltype(m)::value;
            SF_LAUNCH_INST(pair_proj_score_hh_kernel, (MT), dim3(2 * B + nh), block, 0, st, a, g, B, va, sp, B, hh->args, hh->gx);
        }, ints<1, 2, 4>{}));
    }
    if (xn && vphase == 0)
        SF_LAUNCH((pair_proj_score_kernel<0>), dim3(VSP_G * B + B), block, 0, st, a, g, B, va, sp, VSP_G * B);
    else
        SF_LAUNCH((pair_proj_score_kernel<2>), dim3(xn ? 2 * B : B), block, 0, st, a, g, B, va, sp, 0);
    return launch_status();
}

int proj_score_hh_alone(const SmallPlan& hh, hipStream_t st) {
    if (!pair_proj_score_hh_accepts(hh.inst())) return SF_ERR_UNSUPPORTED;
    const int nh = hh.gx * hh.gy;
    return launched(with_index(hh.mt, [&](auto m) {
        constexpr int MT = decltype(m)::value;
        SF_LAUNCH_INST(pair_proj_score_hh_kernel, (MT), dim3(nh), dim3(SMALL_WAVES * 64), 0, st, ProjScoreArgs{}, FGlue{}, 0,
                       VisArgs{}, VisSplit{}, 0, hh.args, hh.gx);
    }, ints<1, 2, 4>{}));
}

// The attention of launches (1) and (2) ALONE, on caller buffers (sf_debug_projected_attention: tests at panorama shapes
// an engine cannot be built for): the same two kernels with empty text, product and scoring parts -- late == 0 the
// partials in launch (1) and their merge in launch (2), else partials, ticket and merge in launch (2).
int proj_attention_alone(const PanoSrc& x, int B, const ProjTables& pt, const float* h1, int ldh1, float* alpha, float* out,
                         int ldo, int late, float* split_part, unsigned* counter, hipStream_t st) {
    if (x.dense || x.half || !x.table || !x.loc_table || !x.vp || !x.view || !pt.pv || !pt.lv || !h1 || !alpha || !out ||
        !split_part)
        return SF_ERR_ARG;
    if (B < 1 || !split_rows_fit(shape(x), B) || !proj_tables_fit(pt.H, pt.ld) || !aligned4(ldh1, ldo) || ldh1 < pt.H ||
        ldo < x.IMG + x.LOC || (late ? !counter : !proj_partials_supported(x.IMG, x.LOC)))
        return SF_ERR_UNSUPPORTED;
    const VisArgs va = proj_vis_args(x, pt, h1, ldh1, alpha, out, ldo, Dropout{}, 0);
    const VisSplit sp{split_part, late ? counter : nullptr, nullptr};
    const dim3 block(SMALL_WAVES * 64);
    if (late) {
        SF_LAUNCH((pair_proj_score_kernel<0>), dim3(VSP_G * B), block, 0, st, ProjScoreArgs{}, FGlue{}, 0, va, sp, VSP_G * B);
    } else {
        SF_LAUNCH((pair_proj_textfold_kernel<1, true>), dim3(PPB_G * B), block, 0, st, va, sp, PPB_G * B, TxtFoldArgs{}, 0,
                  SmallArgs{}, 1);
        SF_LAUNCH((pair_proj_score_kernel<2>), dim3(B), block, 0, st, ProjScoreArgs{}, FGlue{}, 0, va, sp, 0);
    }
    return launch_status();
}

extern "C" void sf_debug_trace(unsigned long long* buf) { g_trace = buf; }
extern "C" void sf_debug_force_write_through(int on) { g_force_sc1 = on; }

// the split visual attention (phase 0: whole, with the ticket inside the launch; 1: partials; 2: merge) beside the small
// product b: the instantiations of VIS_SMALL_INST
int pair_vis_small(const PanoSrc& src, int B, const float* vec, int ldvec, float* alpha, float* out,
                   int ldo, const Dropout& drop, int drop_col0, float* split_part,
                   unsigned* split_counter, const SmallPlan& b, hipStream_t st, int phase) {
    if (!pair_vis_small_accepts(b.inst(), phase)) return SF_ERR_UNSUPPORTED;
    if (!split_part || (phase == 0 && !split_counter) || !split_rows_fit(shape(src), B) || !aligned4(ldvec, ldo))
        return SF_ERR_UNSUPPORTED;
    if (half_misuse(src)) return SF_ERR_ARG;
    VisArgs va{src, vec, ldvec, alpha, out, ldo, drop, drop_col0};
    const int nv = (phase == 2 ? 1 : VSP_G) * B, nb = b.gx * b.gy;
    const dim3 grid(nv + nb), block(SMALL_WAVES * 64);
    const VisSplit sp{split_part, split_counter, g_trace};
    return launched(with_index<VIS_SMALL_INSTS>(vis_small_inst(b.inst(), phase), [&](auto i) {
        constexpr VisSmallInst I = VIS_SMALL_INST[decltype(i)::value];
        constexpr int M = I.mt, C = I.cpw, P = I.phase;
        // (phase 2 only merges partials and never reads the table: its one instantiation serves both storages; the
        //  binary16 name is the one the profile has always reported)
        if constexpr (P != 2) {
            if (src.half) {
                SF_LAUNCH_AS((inst_name<pair_vis_small_kernel<M, C, P, false, true>, M, C, P, false>(
                                 "pair_vis_small_kernel", P ? ", 1 != 2" : ", 0 != 2")),
                             (pair_vis_small_kernel<M, C, P, false, true>), grid, block, 0, st, va, sp, nv, b.args, b.gx);
                return;
            }
        }
        SF_LAUNCH_INST(pair_vis_small_kernel, (M, C, P), grid, block, 0, st, va, sp, nv, b.args, b.gx);
    }));
}

}  // namespace sf

