// The attention dispatch as pure host code: the shape rules of the row-set kernels (visual attention, text attention,
// scoring), what each paired launch accepts of the small products that ride in it, and the ladders that turn a length
// into a template value.  Each rule stands here ONCE: the launchers of sf_attention.hip gate on these predicates and the
// launch chains of sf_api_follower.hip ask the same ones before their first launch.  Nothing here launches or follows a pointer
// and no HIP header is included (tests/test_attention_plan_host.py compiles it with g++).  DESIGN.md: "Attention
// dispatch: rules and ladders".
#pragma once
#include <cstddef>

#include "sf_gemm_plan.h"

namespace sf {

// ---- the tile constants the rules read (the kernels of sf_attention.hip include this file: one definition) ------------
constexpr int VIS_CPL = 9, VIS_RPW = 3, VIS_NW = 12, VIS_SLOTS = 6;   // visual attention: float4 per lane, rows per wave, waves
#ifndef SF_VIS_GROUPS
#define SF_VIS_GROUPS 2
#endif
constexpr int VSP_G = SF_VIS_GROUPS;                   // split visual attention: workgroups per sample (2 or 4)
constexpr int VSP_NW = VIS_NW / VSP_G, VSP_RPG = VSP_NW * VIS_RPW, VSP_SLOTS = VSP_NW < 3 ? VSP_NW : 3;
static_assert(VSP_G == 2 || VSP_G == 4, "ticket arithmetic assumes a power of two");
// Largest batch of the split visual attention (per-sample ticket counters) and of the schedules built around it: the
// paired / folded decode steps and the two-stream backward through time (sf_follower_episode_bwd).  Above it the
// un-split kernels run and those schedules fall back to one launch at a time on one stream.
constexpr int VIS_SPLIT_MAX_B = 256;
constexpr int PRJ_CPL = 2;                             // float4 per lane of a projected row: H <= 512
constexpr int PPB_G = 3;                               // projected partials: workgroups per sample
constexpr int SPLIT_MAX_G = PPB_G > VSP_G ? PPB_G : VSP_G;      // records per sample the split scratch is sized for
constexpr int TXT_CPL = 2, TXT_NW = 16, TXT_SLOTS = 8; // text attention
constexpr int TXT_MAX_L = TXT_NW * 8;
constexpr int SC_CPL = 9, SC_NW = 16, SC_SLOTS = 4;    // scoring
constexpr int TXF_G = 4;          // folded text: workgroups per sample; tickets a LAUNCH adds per sample (they count in fours)
constexpr int TXF_MAX_L = TXF_G * SMALL_WAVES * 5, TXF_MAX_B = 512;
constexpr int TXF_G2_MAX_L = 2 * SMALL_WAVES * 5;      // ... in two groups (proj_text_groups_plan)
constexpr int CG_ROWS = 10;                            // ctx_grad_kernel: rows per thread, L <= 8 * CG_ROWS
static_assert(SC_NW == 2 * SMALL_WAVES, "the projected scoring (two rows per wave of a small block) takes the candidate rule");

// ---- shape rules --------------------------------------------------------------------------------------------------------
// a row source (PanoSrc / CandSrc of sf_rows.h) as the rules see it: rows = V or A
struct RowShape {
    int rows, IMG, LOC;
    bool dense, half;
};
inline bool aligned4(int a, int b = 0, int c = 0) { return ((a | b | c) & 3) == 0; }
// rows of F = IMG + LOC floats in `cpl` float4 per lane; the index form reads the two parts in chunks of their own
inline bool row_width_fits(const RowShape& s, int cpl, int loc_multiple) {
    const int F = s.IMG + s.LOC;
    return F <= cpl * 256 && aligned4(F) && (s.dense || (aligned4(s.IMG) && s.LOC % loc_multiple == 0));
}
// the panorama rows fit the registers of a visual-attention block
inline bool pano_rows_fit(const RowShape& s) { return s.rows <= VIS_RPW * VIS_NW && s.rows <= 64 && row_width_fits(s, VIS_CPL, 4); }
// within the range of the VSP_G-workgroup split (a smaller V leaves a group without rows)
inline bool in_split_range(int V, int B) { return V > (VSP_G - 1) * VSP_RPG && V <= VSP_G * VSP_RPG && B <= VIS_SPLIT_MAX_B; }
// the candidate rows fit a scoring block; the index form repeats sin / cos over LOC / 4 columns each, in float4: LOC % 16
inline bool cand_rows_fit(const RowShape& s) { return s.rows >= 1 && s.rows <= SC_NW && row_width_fits(s, SC_CPL, 16); }
// the context rows fit a text-attention block of up to Lmax positions; lds: the leading dimensions, or-ed
inline bool text_rows_fit(int L, int Lmax, int H, int lds) { return H <= TXT_CPL * 256 && aligned4(H, lds) && L >= 1 && L <= Lmax; }
// ... and the folded text stage, whose merged sum goes to z [B, ldz]
inline bool text_fold_fits(int B, int L, int H, int ldvec, int ldz) {
    return text_rows_fit(L, TXF_MAX_L, H, ldvec | ldz) && B <= TXF_MAX_B && ldz >= H;
}
// both: what every split launch asks of its panorama (and visual_attn_f64_supported: the float64 scores exist split only)
inline bool split_rows_fit(const RowShape& s, int B) { return pano_rows_fit(s) && in_split_range(s.rows, B); }
inline bool ctx_grad_supported(int S, int L, int H) {
    const int n4 = H >> 2;
    return !(H & 3) && n4 >= 1 && n4 <= 1024 && 1024 % n4 == 0 && L <= (1024 / n4) * CG_ROWS &&
           (size_t)S * 2 * L * sizeof(float) <= 64 * 1024;
}
// the projected tables [., ld] of a decoder of width H (sf_projected_build)
inline bool proj_tables_fit(int H, int ld) { return H <= PRJ_CPL * 256 && aligned4(H, ld) && H >= 4 && ld >= H + 1; }
// the projected decode chain: index-form fp32 candidates `us`; `xn` (or null) the panorama whose attention rides along
inline bool proj_chain_supported(const RowShape& us, const RowShape* xn, int B, int H, int L, int tables_H, int tables_ld) {
    if (tables_H != H || !proj_tables_fit(H, tables_ld) || L < 1 || L > TXF_MAX_L || B < 1 || B > VIS_SPLIT_MAX_B) return false;
    if (us.dense || us.half || !cand_rows_fit(us)) return false;
    return !xn || (!xn->dense && !xn->half && xn->IMG == us.IMG && xn->LOC == us.LOC && split_rows_fit(*xn, B));
}
// whether launch (1) of that chain can carry the partials of a panorama (else they ride in launch (2), vphase 0):
// proj_partials_body types a lane's VIS_CPL row slots as image or location chunks, both parts must fit side by side
inline bool proj_partials_supported(int IMG, int LOC) { return IMG >= 4 && ((IMG >> 2) + 63) / 64 + ((LOC >> 2) + 63) / 64 <= VIS_CPL; }

// ---- scratch sizes ------------------------------------------------------------------------------------------------------
// (sized for the body with the most records per sample: proj_partials_body and proj_merge_body index the same scratch
//  with PPB_G records, every visual_split_body with VSP_G)
inline size_t visual_attn_split_floats(int B, int F) { return (size_t)B * SPLIT_MAX_G * (F + 64); }
inline size_t text_fold_part_floats(int B, int H) { return (size_t)B * TXF_G * (H + 64); }

// ---- ladders: the template value of a length (0: none) ------------------------------------------------------------------
inline int text_rpw(int L) { return L <= TXT_NW ? 1 : L <= TXT_NW * 5 ? 5 : L <= TXT_MAX_L ? 8 : 0; }             // text_attn_kernel
// the folded text stage in G groups of SMALL_WAVES waves: rung 0 .. 3 = 1, 2, 3, 5 positions per wave
inline int text_rung(int L, int G) {
    const int rpw = (L + G * SMALL_WAVES - 1) / (G * SMALL_WAVES);
    return rpw <= 1 ? 0 : rpw <= 2 ? 1 : rpw <= 3 ? 2 : 3;
}
constexpr int FOLD_RPW[4] = {1, 2, 3, 5};
inline int fold_rpw(int L, int G) { return FOLD_RPW[text_rung(L, G)]; }

// ---- text groups per sample of launch (1) of the projected chain.  With the partials the kernel holds proj_partials_body's
// ~125 registers, two workgroups per CU: at batch 100 the four-group grid (300 + 400 + 224 blocks: the y product plans
// (mt 1, cpw 4), a 32 x 7 grid, not the 32 blocks earlier notes counted) is 924 blocks on 512 resident slots, and the
// text groups of the second round pay their load -> reduce -> ticket -> merge latency behind a first-round block, on the
// chain cell -> text -> score -> next gate product.  TWO groups of 8 * RPW positions (RPW <= 5: L <= 80) make it 724: every
// text group starts in the first round, 212 of the y blocks in a second.  The rule is a pure function of (B, L, device) -- a captured replay and an eager rollout of one
// shape choose alike: two groups iff the partials ride in this launch, L <= 80, and the four-group grid exceeds the
// resident slots.  force (sf_debug_projected_text_groups): 0 the rule, 2 / 4 that count where it is legal.  na: blocks of
// the y product, slots: resident workgroups of the four-group launch (0: unknown).
inline int proj_text_groups_plan(int B, int L, bool with_partials, int na, int slots, int force, int* grid) {
    const int nv = with_partials ? PPB_G * B : 0;
    const bool legal = with_partials && L <= TXF_G2_MAX_L;
    const bool crowded = slots > 0 && nv + TXF_G * B + na > slots;
    const int G = legal && (force == 2 || (force != TXF_G && crowded)) ? 2 : TXF_G;
    if (grid) *grid = nv + G * B + na;
    return G;
}

// ---- what a paired launch accepts of its small products' (mt, cpw): the instantiations of its kernel ------------------
inline bool mt_124(int mt) { return mt == 1 || mt == 2 || mt == 4; }
inline bool pair_small_small_accepts(SmallInst a, SmallInst b) { return a.mt == 1 && a.cpw == 4 && b.cpw == 4 && mt_124(b.mt); }
// (y and t_v' of the four-launch folded chain: t_v' has the shape of t_a, which pair_apro_small takes as (1, 4) only)
inline bool pair_textfold_small_small_accepts(SmallInst a, SmallInst b) { return a.mt == 1 && a.cpw == 4 && b.mt == 1 && b.cpw == 4; }
inline bool pair_proj_textfold_accepts(SmallInst y) { return y.mt == 1 && y.cpw == 4; }
// launch (2)'s product blocks (the next step's h1 W_hh^T + biases, K = H <= 512: four chunks per wave)
inline bool pair_proj_score_hh_accepts(SmallInst hh) { return hh.cpw == 4 && mt_124(hh.mt); }
inline bool pair_apro_small_accepts(SmallInst a, SmallInst b) { return a.mt == 1 && a.cpw == 4 && b.cpw == 2 && mt_124(b.mt); }
inline bool pair_small_text_accepts(SmallInst a) { return a.mt == 4 && a.cpw == 2; }
inline bool pair_visbwd_small_accepts(SmallInst b) { return b.mt == 1 && b.cpw == 16; }     // the K = 4H recurrent data gradient
// pair_vis_small_kernel<MT, CPW, PHASE>: beside the partials (phases 0, 1) the r = W_a^T wt product of the folded text
// chain (K = D = 256: two chunks per wave) or a one-tile-row product of eight; beside the merge (phase 2) one of eight or four
struct VisSmallInst { int mt, cpw, phase; };
constexpr int VIS_SMALL_INSTS = 10;
constexpr VisSmallInst VIS_SMALL_INST[VIS_SMALL_INSTS] = {
    {1, 2, 0}, {2, 2, 0}, {4, 2, 0}, {1, 8, 0}, {1, 2, 1}, {2, 2, 1}, {4, 2, 1}, {1, 8, 1}, {1, 8, 2}, {1, 4, 2}};
constexpr int vis_small_inst(SmallInst b, int phase) {        // position in the table (past its end: no such instantiation)
    int i = 0;
    while (i < VIS_SMALL_INSTS && (VIS_SMALL_INST[i].mt != b.mt || VIS_SMALL_INST[i].cpw != b.cpw || VIS_SMALL_INST[i].phase != phase)) ++i;
    return i;
}
inline bool pair_vis_small_accepts(SmallInst b, int phase) { return vis_small_inst(b, phase) < VIS_SMALL_INSTS; }

}  // namespace sf
