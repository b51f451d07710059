// The rules, ladders and acceptance predicates of csrc/sf_attention_plan.h behind a C interface, for
// tests/test_attention_plan_host.py: compiled with g++ alone (the header includes no HIP header), loaded with ctypes.
#include "sf_attention_plan.h"

using namespace sf;

// s: rows, IMG, LOC, dense, half
static RowShape shape(const int* s) { return RowShape{s[0], s[1], s[2], s[3] != 0, s[4] != 0}; }

extern "C" {

// out: the constants tests/attention_cases.py mirrors, then the other tile constants a rule reads; returns the count
int shim_tables(int* out) {
    const int v[] = {VIS_CPL, VIS_RPW, VIS_NW, VSP_G, VSP_RPG, VIS_SPLIT_MAX_B, TXT_CPL, TXT_NW, SC_CPL, SC_NW, CG_ROWS,
                     TXT_MAX_L, TXF_G, TXF_MAX_L, TXF_MAX_B, TXF_G2_MAX_L, PRJ_CPL, PPB_G, SPLIT_MAX_G, SMALL_WAVES};
    const int n = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return n;
}

int shim_pano_rows_fit(const int* s) { return pano_rows_fit(shape(s)); }
int shim_in_split_range(int V, int B) { return in_split_range(V, B); }
int shim_split_rows_fit(const int* s, int B) { return split_rows_fit(shape(s), B); }
int shim_cand_rows_fit(const int* s) { return cand_rows_fit(shape(s)); }
int shim_aligned4(int a, int b, int c) { return aligned4(a, b, c); }
int shim_text_rows_fit(int L, int Lmax, int H, int lds) { return text_rows_fit(L, Lmax, H, lds); }
int shim_text_fold_fits(int B, int L, int H, int ldvec, int ldz) { return text_fold_fits(B, L, H, ldvec, ldz); }
int shim_ctx_grad_supported(int S, int L, int H) { return ctx_grad_supported(S, L, H); }
int shim_proj_tables_fit(int H, int ld) { return proj_tables_fit(H, ld); }
// xn null: no panorama rides along
int shim_proj_chain_supported(const int* us, const int* xn, int B, int H, int L, int tables_H, int tables_ld) {
    const RowShape x = xn ? shape(xn) : RowShape{};
    return proj_chain_supported(shape(us), xn ? &x : nullptr, B, H, L, tables_H, tables_ld);
}
int shim_proj_partials_supported(int IMG, int LOC) { return proj_partials_supported(IMG, LOC); }
long long shim_visual_attn_split_floats(int B, int F) { return (long long)visual_attn_split_floats(B, F); }
long long shim_text_fold_part_floats(int B, int H) { return (long long)text_fold_part_floats(B, H); }

int shim_text_rpw(int L) { return text_rpw(L); }
int shim_text_rung(int L, int G) { return text_rung(L, G); }
int shim_fold_rpw(int L, int G) { return fold_rpw(L, G); }
int shim_proj_text_groups_plan(int B, int L, int with_partials, int na, int slots, int force, int* grid) {
    return proj_text_groups_plan(B, L, with_partials != 0, na, slots, force, grid);
}

// which: 0 pair_small_small, 1 pair_textfold_small_small, 2 pair_apro_small (products a and b); 3 pair_small_text,
// 4 pair_visbwd_small, 5 pair_proj_textfold (product a); 6 pair_vis_small (product a, phase)
int shim_accepts(int which, int amt, int acpw, int bmt, int bcpw, int phase) {
    const SmallInst a{amt, acpw}, b{bmt, bcpw};
    switch (which) {
        case 0: return pair_small_small_accepts(a, b);
        case 1: return pair_textfold_small_small_accepts(a, b);
        case 2: return pair_apro_small_accepts(a, b);
        case 3: return pair_small_text_accepts(a);
        case 4: return pair_visbwd_small_accepts(a);
        case 5: return pair_proj_textfold_accepts(a);
        case 6: return pair_vis_small_accepts(a, phase);
    }
    return -1;
}
// the instantiations of pair_vis_small_kernel as (mt, cpw, phase) triples; returns their number
int shim_vis_small_insts(int* out) {
    for (int i = 0; i < VIS_SMALL_INSTS; ++i) {
        out[3 * i] = VIS_SMALL_INST[i].mt; out[3 * i + 1] = VIS_SMALL_INST[i].cpw; out[3 * i + 2] = VIS_SMALL_INST[i].phase;
    }
    return VIS_SMALL_INSTS;
}

}  // extern "C"
