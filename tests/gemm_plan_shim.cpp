// The plan functions of csrc/sf_gemm_plan.h behind a C interface, for tests/test_gemm_plan_host.py: compiled with g++ alone
// (the header includes no HIP header), loaded with ctypes.  Every plan comes back as a flat array of 64-bit integers.
#include "sf_gemm_plan.h"

using namespace sf;
typedef long long i64;

// sw: force_f32, big, big_ksplit, tn_split_min_rows, tn_group
static GemmSwitches switches(const int* sw) { return GemmSwitches{sw[0], sw[1], sw[2], sw[3], sw[4]}; }

static i64* put_part(i64* o, const TnPart& p) {
    *o++ = p.family; *o++ = p.splits; *o++ = p.grid.x; *o++ = p.grid.y; *o++ = p.grid.z;
    *o++ = (i64)p.off_xt; *o++ = (i64)p.off_slabs; *o++ = (i64)p.ws_floats;
    return o;
}

struct ShimJob { int M, P, Q, ldy, ldx; i64 Y, X; };      // Y, X: numbers that stand for the operands

extern "C" {

// out: the (MT, CPW) pairs of the short-reduction kernel, then NT_MT_MAX, then the MT of gemm_nn_kernel; returns the count
int shim_tables(int* out) {
    int n = 0;
    for (int i = 0; i < SMALL_INSTS; ++i) { out[n++] = SMALL_INST[i].mt; out[n++] = SMALL_INST[i].cpw; }
    out[n++] = NT_MT_MAX;
    for (int i = 0; i < NN_INSTS; ++i) out[n++] = NN_INST[i];
    return n;
}

// flags: raw_slabs, ksplit_out, packed_w, epi, accumulate, addend, r1_s
// out: status, family, mt, cpw, extras, grid x y z, block, lds, ksplit, slabs, reduce, ws_floats
void shim_plan_nt(int M, int N, const int* K, int nseg, const int* flags, i64 ws_floats, const int* sw, i64* out) {
    NtAsk q{};
    q.M = M; q.N = N; q.nseg = nseg;
    for (int s = 0; s < nseg; ++s) q.K[s] = K[s];
    q.raw_slabs = flags[0]; q.ksplit_out = flags[1]; q.packed_w = flags[2]; q.epi = flags[3];
    q.accumulate = flags[4]; q.addend = flags[5]; q.r1_s = flags[6];
    q.ws_floats = (size_t)ws_floats;
    const NtPlan p = plan_nt(q, switches(sw));
    const i64 v[14] = {p.status, p.family, p.mt, p.cpw, p.extras, p.grid.x, p.grid.y, p.grid.z, p.block, (i64)p.lds,
                       p.ksplit, p.slabs, p.reduce, (i64)p.ws_floats};
    for (int i = 0; i < 14; ++i) out[i] = v[i];
}

// out: mt, mblocks, ks, grid x y z, ws_floats, gemm_nn_ws_floats(M, N, K)
void shim_plan_nn(int M, int N, int K, i64 ws_floats, i64* out) {
    const NnPlan p = plan_nn(M, N, K, (size_t)ws_floats);
    const i64 v[8] = {p.mt, p.mblocks, p.ks, p.grid.x, p.grid.y, p.grid.z, (i64)p.ws_floats, (i64)gemm_nn_ws_floats(M, N, K)};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}

// out: the plan, its main and its tail part (family, splits, grid x y z, off_xt, off_slabs, ws_floats each), q_main,
// gemm_tn_main_columns(M, P, Q)
void shim_plan_tn(int M, int P, int Q, int ldy, i64 ws_floats, const int* sw, i64* out) {
    const TnPlan p = plan_tn(M, P, Q, ldy, (size_t)ws_floats, switches(sw));
    out = put_part(put_part(put_part(out, p), p.main), p.tail);
    *out++ = p.q_main;
    *out++ = gemm_tn_main_columns(M, P, Q);
}

// out: grouped, n, ntr, reduce, most, ws_floats; then per grouped job (NB_GROUP of them) job, ks, yt, xt, off_slabs; then per
// transpose (TR_GROUP of them) job, x, off.  Returns the number of values.
int shim_plan_tn_group(const ShimJob* jobs, int n, i64 ws_floats, const int* sw, i64* out) {
    const TnGroupPlan g = plan_tn_group(jobs, n, (size_t)ws_floats, switches(sw));
    i64* o = out;
    *o++ = g.grouped; *o++ = g.n; *o++ = g.ntr; *o++ = g.reduce; *o++ = (i64)g.most; *o++ = (i64)g.ws_floats;
    for (int k = 0; k < NB_GROUP; ++k) { *o++ = g.job[k]; *o++ = g.ks[k]; *o++ = g.yt[k]; *o++ = g.xt[k]; *o++ = (i64)g.off_slabs[k]; }
    for (int j = 0; j < TR_GROUP; ++j) { *o++ = g.tr[j].job; *o++ = g.tr[j].x; *o++ = (i64)g.tr[j].off; }
    return (int)(o - out);
}

// out: ms, grid x y, finish x, ws_floats
void shim_plan_colsum(int M, int N, i64 ws_floats, i64* out) {
    const ColsumPlan p = plan_colsum(M, N, (size_t)ws_floats);
    const i64 v[5] = {p.ms, p.grid.x, p.grid.y, p.finish.x, (i64)p.ws_floats};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
}

}  // extern "C"
