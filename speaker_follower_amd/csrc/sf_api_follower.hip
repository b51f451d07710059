// The follower's decode step (a6), software-pipelined across steps, as its five launch chains; the whole episode forward
// and backward in one call each; the stacked weight gradients, the follower glue and its loss.  Host sequencing only
// (sf_api_util.h): nothing here allocates or synchronises.
#include "sf_api_util.h"

#include <map>
#include <vector>

using namespace sf;

namespace {

// ---- a6, software-pipelined across steps ---------------------------------------------------------------
// head(t)   = visual half of step t: t_v, q, visual attention -> tape->xin[:, F:2F], alpha_v
// tail(t)   = LSTM cell, text attention, scoring (+ glue) of step t, and -- when X_next is given --
//             head(t+1) on h1 of step t, run SIDE BY SIDE with the text / scoring half in paired
//             launches (sf_attention.hip): the two halves are independent given h1.
int decoder_head_a(const sf_decoder_w* w, const sf_pano* X, int B, int H, int D,
                   const float* h0, const sf_decoder_tape* tp, const sf_dropout* drop,
                   uint32_t step_id, Arena ar, sf_stream stream) {
    SF_CHECK_ARG(w && X && h0 && tp && B > 0);
    const PanoSrc xs = pano(X);
    const int F = xs.IMG + xs.LOC;
    return visual_fwd_i(&w->visual, xs, B, H, D, h0, tp->xin + F, 2 * F, tp->alpha_v, tp->t_v, tp->q,
                        make_dropout(drop, 2 * step_id, 2), F, ar, S(stream));
}

int plan_linear(const float* x, int ldx, const float* wgt, int ldw, const float* b, int M,
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

// Gate-space rows through one step (sf_follower_episode_fwd): `xg_in` is the row the step before left for this step's cell
// (null: the full gate product), `rows.xg_next` where launch (2) of the projected chain leaves the next one; `wrote` says
// whether it did -- any other chain writes the raw u_next alone, and the next step runs the full product.
// The attended half (sf_gate_rows_attended_build) rides on that: `xg_f_in` is the [B, 4H] row launch (2) of the step before
// merged from gate-space partials (null: the raw attended feature is in xin, as without the table; never set without
// `xg_in`), `rows.gf` / `rows.xg_f` the table and where this step's launch (2) leaves the next one, `wrote_f` whether it did.
// The recurrent half (sf_gate_rows_recurrent_use) rides on both: `xg_h_in` is the [B, 4H] row h0 W_hh^T + b_ih + b_hh the
// product blocks of launch (2) of the step before formed (null: the cell forms it; never set without `xg_f_in`),
// `rows.xg_h` where this step's launch (2) leaves the next one, `wrote_h` whether it did.
struct GateStep {
    const float* xg_in;
    GateRows rows;
    bool wrote;
    const float* xg_f_in = nullptr;
    bool wrote_f = false;
    const float* xg_h_in = nullptr;
    bool wrote_h = false;
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
    GateStep* gate;                     // gate-space rows of the episode (null: none), see GateStep
};

// a launch BEHIND a chain's first one: the step is half issued, "unsupported" can no longer mean "try the next chain"
inline int issued(int rc) { return rc == SF_ERR_UNSUPPORTED ? SF_ERR_LAUNCH : rc; }

// the second body of a paired launch left empty (no next step to prepare)
SmallPlan empty_plan(SmallPlan p) {
    p.gx = p.gy = 0;
    return p;
}

// the visual attention of step t+1 on its query tn->q -- beside the small product `b` (phases: pair_vis_small) ...
int vis_next_beside(const TailStep& s, float* part, unsigned* counter, const SmallPlan& b, int phase = 0) {
    return pair_vis_small(s.xn, s.B, s.tn->q, s.F, s.tn->alpha_v, s.tn->xin + s.F, 2 * s.F, s.dn_in, s.F, part, counter, b,
                          s.st, phase);
}
// ... or as a launch of its own
int vis_next_alone(const TailStep& s, float* part, const Arena& ar) {
    return visual_attn(0, s.xn, s.B, s.tn->q, s.F, s.tn->alpha_v, s.tn->xin + s.F, 2 * s.F, s.dn_in, s.F, s.st, part,
                       part ? ar.tickets() : nullptr);
}

int score_tail(const TailStep& s, const Arena& ar, bool t_a_done = false) {
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
FoldScratch fold_scratch(const TailStep& s, Arena& af) {
    FoldScratch f{};
    f.tpart = af.take(text_fold_part_floats(s.B, s.H));
    // (leading dimension H + 16: rows of a power-of-two stride share a few cache sets, CHANGELOG round 5 "2c")
    f.ldp = s.H + 16;
    f.ybuf = af.take((size_t)s.B * f.ldp);
    f.zbuf = af.take((size_t)s.B * f.ldp);
    f.tcount = af.tickets() ? af.tickets() + TEXT_TICKET : nullptr;
    // (with gate-space rows for the attended half a record holds 4H + LOC floats: sized for the larger of the two widths)
    const int width = s.gate && s.gate->rows.gf && s.paired ? std::max(s.F, 4 * s.H + s.xn.LOC) : s.F;
    f.part = (s.paired && s.B <= 1024) ? af.take(visual_attn_split_floats(s.B, width)) : nullptr;
    f.ok = f.tpart && f.ybuf && f.zbuf && (f.part || !s.paired) && f.tcount && s.B <= VIS_SPLIT_MAX_B;
    return f;
}

// the last launch of the four-launch folded chain: logit = u . r + the biases through wt -- with the glue and the merge of
// the next step's attention partials `merge_part` in the same launch, with the glue alone, or bare
int fold_score(const TailStep& s, float* merge_part) {
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
bool projected_for(const sf_decoder_w* w, const CandSrc& us, const PanoSrc* xn, int B, int H, int L, ProjTables* pt) {
    sf_projected reg;
    if (us.dense || us.half || !projected_lookup(us.table, &reg)) return false;
    if (reg.key_v != w->visual.w_h || reg.key_a != w->action.w_h || reg.V != us.V || reg.IMG != us.IMG || reg.LOC != us.LOC ||
        (xn && xn->loc_table != reg.loc_table))
        return false;
    *pt = ProjTables{reg.pv, reg.pa, reg.lv, reg.la, reg.ld, reg.H};
    return proj_chain_supported(us, xn, B, H, L, *pt);
}

int tail_proj(const TailStep& s, const TextFold& tf) {
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
    const bool gate = s.gate && s.gate->rows.xg_next && s.paired;       // (a next step exists and reads the row)
    // the attended half in gate space: only beside the action half's row, with the partials in launch (1), and where their
    // body takes rows of 4H + LOC floats (episode_gate_rows has checked the table and the shape of what is left)
    const bool att = gate && !late && s.gate->rows.gf && s.gate->rows.xg_f && !s.dn_in.on() &&
                     proj_partials_supported(4 * H, s.xn.LOC);
    GateRows rows = gate ? s.gate->rows : GateRows{};
    if (!att) rows.gf = nullptr, rows.xg_f = nullptr, rows.xg_h = nullptr;
    // the recurrent half of the next step's gates as product blocks of launch (2): only beside both rows, where
    // episode_gate_rows carved the row (switch, shape of the cell behind, capacity) and the plan is one launch (2) takes --
    // planned HERE, ahead of launch (1): without a plan the step runs without the row, it is never left half issued
    SmallPlan phh;
    if (rows.xg_h) {
        Seg sg{tp->h1, H, s.w->lstm.w_hh, H, H};
        LinearOut o{};
        o.y = rows.xg_h; o.ldy = 4 * H; o.bias = s.w->lstm.b_ih; o.bias2 = s.w->lstm.b_hh; o.epi = EPI_NONE;
        if (!linear_small_plan(&sg, 1, B, 4 * H, o, &phh) || !pair_proj_score_hh_accepts(phh.inst())) rows.xg_h = nullptr;
    }
    const bool rec = rows.xg_h != nullptr;
    TRY(pair_proj_textfold(tf.ctx_q, tf.ctx_o, s.ctx_mask, B, s.L, H, tp->cat2 + H, 2 * H, f.tpart, f.tcount, f.zbuf, f.ldp,
                           tp->alpha, py, s.us, s.paired && !late ? &s.xn : nullptr, pt, tp->h1, H, f.part, s.st, rows.gf));
    g_proj_steps.fetch_add(1, std::memory_order_relaxed);
    TRY(issued(pair_proj_score(s.us, B, H, s.L, pt, f.zbuf, f.ldp, f.ybuf, f.ldp, make_glue(s.us, B, tp->logit, s.glue),
                               s.paired ? &s.xn : nullptr, late ? 0 : 2, tp->h1, H, s.paired ? tn->alpha_v : nullptr,
                               s.paired ? tn->xin + F : nullptr, 2 * F, s.dn_in, F, f.part, af.tickets(), s.st,
                               gate ? &rows : nullptr, rec ? &phh : nullptr)));
    if (gate) s.gate->wrote = true;
    if (att) s.gate->wrote_f = true;
    if (rec) s.gate->wrote_h = true;
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
int tail_fold4(const TailStep& s, const TextFold& tf) {
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
int text_and_query(const TailStep& s) {
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
int tail_paired(const TailStep& s) {
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
int tail_query_only(const TailStep& s) {
    const sf_decoder_tape* tp = s.tp;
    TRY(text_and_query(s));
    TRY(linear_plain(tp->cat2, 2 * s.H, s.w->text.w_out, 2 * s.H, nullptr, s.B, s.H, 2 * s.H, EPI_TANH, tp->h_tilde, s.H,
                     s.ar, s.st));
    return score_tail(s, s.ar);
}

// The plain step: text attention and scoring, and -- with a next panorama but no transposed W_v to pair its query
// with -- the whole visual half of step t+1 behind them.
int tail_plain(const TailStep& s) {
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
int tail_dispatch(const TailStep& s, const TextFold* tf) {
    const bool foldable = (s.paired || s.query_only || s.last_step) && tf && !s.ctx_row && !s.d_h.on() && s.w->text.w_out;
    int rc = SF_ERR_UNSUPPORTED;
    if (foldable) rc = tail_proj(s, *tf);
    if (rc == SF_ERR_UNSUPPORTED && foldable && s.w->action.w_a_t) rc = tail_fold4(s, *tf);
    if (rc != SF_ERR_UNSUPPORTED) return rc;
    if (s.paired) return tail_paired(s);
    if (s.query_only) return tail_query_only(s);
    return tail_plain(s);
}

int decoder_tail_i(const sf_decoder_w* w, const sf_cands* U, int B, int H, int D, int L,
                   const float* u_prev, const float* h0, const float* c0, const float* ctx,
                   const uint8_t* ctx_mask, const int32_t* ctx_row, const sf_decoder_tape* tp,
                   const sf_follower_glue* glue, const sf_dropout* drop, uint32_t step_id,
                   const sf_pano* X_next, const sf_decoder_tape* tn, Arena ar, hipStream_t st,
                   const TextFold* tf = nullptr, GateStep* gate = nullptr) {
    SF_CHECK_ARG(w && U && h0 && c0 && ctx && tp && B > 0 && L > 0 && (!glue || glue_ok(U, glue)) &&
                 (!X_next || tn));
    TailStep s{};
    s.gate = gate;
    s.w = w; s.us = cands(U); s.B = B; s.H = H; s.D = D; s.L = L; s.F = s.us.IMG + s.us.LOC;
    s.tp = tp; s.tn = tn; s.glue = glue;
    s.ctx = ctx; s.ctx_mask = ctx_mask; s.ctx_row = ctx_row;
    s.ar = ar;
    s.st = st;
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
    // (with a row of the attended half's image part too: the product over [f_loc | h0], K = LOC + H, both rows added)
    const float* xg_f = xg ? gate->xg_f_in : nullptr;
    // (with the recurrent half and the biases as a third row: the product over f_loc alone, K = LOC, three rows added)
    const float* xg_h = xg_f ? gate->xg_h_in : nullptr;
    TRY(lstm_fwd_i(&w->lstm, B, 2 * s.F, H, tp->xin, 2 * s.F, h0, c0, tp->h1, tp->c1, tp->gates,
                   tp->cat2 + H, 2 * H, s.d_h, s.ar, s.st, xg, xg_f ? s.F + s.us.IMG : s.F, xg_f, 0, xg_h));
    if (xg) g_gate_steps.fetch_add(1, std::memory_order_relaxed);
    if (xg_f) g_gate_att_steps.fetch_add(1, std::memory_order_relaxed);
    if (xg_h) g_gate_rec_steps.fetch_add(1, std::memory_order_relaxed);
    return tail_dispatch(s, tf);
}

// the visual attention of a step on the query its tape holds already (sf_attn_decoder_attend_fwd)
int attend_i(const sf_pano* X, int B, const sf_decoder_tape* tp, const sf_dropout* drop, uint32_t step_id, Arena ar,
             hipStream_t st) {
    SF_CHECK_ARG(X && tp && tp->q && tp->xin && tp->alpha_v && B > 0);
    const PanoSrc xs = pano(X);
    const int F = xs.IMG + xs.LOC;
    float* part = B <= 1024 ? ar.take(visual_attn_split_floats(B, F)) : nullptr;
    return visual_attn(0, xs, B, tp->q, F, tp->alpha_v, tp->xin + F, 2 * F, make_dropout(drop, 2 * step_id, 2), F,
                       st, part, part ? ar.tickets() : nullptr);
}

// The backward of one decode step is two chains that only meet at the LSTM pointwise backward:
//   head: scoring -> h~ -> text attention  =>  dh1d (the attention path's share of d h1), and the dY
//         operands of that half; needs only the forward tape and d(logit) of ITS step;
//   tail: LSTM cell -> input gradient -> visual attention  =>  dh0, dc0; needs dh1 / dc1 of step t+1.
// So head(t-1) can run while tail(t) does (sf_follower_episode_bwd puts the heads on a side stream).
int decoder_bwd_head_i(const sf_decoder_w* w, const sf_decoder_g* g, const sf_cands* U, int B,
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

int decoder_bwd_tail_i(const sf_decoder_w* w, const sf_decoder_g* g, const sf_pano* X, int B,
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

int decoder_bwd_i(const sf_decoder_w* w, const sf_decoder_g* g, const sf_pano* X,
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

// ---- a whole follower episode (follower.py:430-539 / 1001-1020) in one call ----------------------------
// Every per-step tensor of an index-form episode is a stacked [S][...] array, so the decode loop and
// its backward need no host work between steps: the host mirror makes ONE call instead of 2 S (its
// Python + ctypes cost per step was exposed as idle gaps between the short kernels of the backward).

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

// ---- sf_follower_episode_fwd in its four parts -------------------------------------------------------------------------
// What the parts read of the episode beyond the struct itself: step 0's sources (converted ONCE), the dropout and the
// device-resident environment where there is one, and -- set by part (1) -- the folded context.
struct EpisodeFwd {
    const sf_decoder_w* w;
    const sf_follower_episode* e;
    const sf_dropout* drop;          // null: none
    const sf_nav_io* nav0;           // sf_nav_io of step 0 (null: the panoramas are the caller's)
    StepView cur;                    // step 0
    PanoSrc x0;
    CandSrc us0;
    TextFold fold;
    const TextFold* tf;              // &fold once part (1) has formed it (null: the unfolded chains)
    sf_stream stream;
};

// (1) the folded text attention (ABI 9): ctx_q = ctx W_in, ctx_o = ctx W_out[:, :H]^T, once per episode
int episode_text_fold(EpisodeFwd& ep, Arena ar) {
    const sf_follower_episode* e = ep.e;
    const sf_decoder_w* w = ep.w;
    const sf_dropout* drop = ep.drop;
    if (e->ctx_q && e->ctx_o && !drop && e->S > 1 && w->text.w_in_t && w->text.w_out && w->action.w_a_t) {
        TRY(context_fold(e->ctx, w->text.w_in_t, w->text.w_out, e->B * e->L, e->H, e->ctx_q, e->ctx_o, ar, S(ep.stream)));
        ep.tf = &ep.fold;
    }
    return SF_OK;
}

// (2) step 0's head.  The projected chain's: attention straight from h_init through the projected rows, ONE launch
// instead of t_v', q' and the attention (same conditions as the steps: tail_proj); or decoder_head_a
int episode_head(const EpisodeFwd& ep, Arena ha) {
    const sf_follower_episode* e = ep.e;
    const sf_decoder_w* w = ep.w;
    const sf_dropout* drop = ep.drop;
    const TextFold* tf = ep.tf;
    const StepView& cur = ep.cur;
    const PanoSrc& x0 = ep.x0;
    ProjTables pt;
    float* part = nullptr;
    if (tf && !e->glue.nav && e->B <= VIS_SPLIT_MAX_B && projected_for(w, ep.us0, &x0, e->B, e->H, e->L, &pt) &&
        (part = ha.take(visual_attn_split_floats(e->B, x0.IMG + x0.LOC))) && ha.tickets()) {
        const int F = x0.IMG + x0.LOC;
        const int rc = visual_attn_proj(ep.us0, x0, e->B, e->H, e->L, pt, e->h_init, e->H, cur.tp.alpha_v,
                                        cur.tp.xin + F, 2 * F, make_dropout(drop, 2 * e->step0, 2), F, part, ha.tickets(),
                                        S(ep.stream));
        if (rc != SF_ERR_UNSUPPORTED) return rc;
    }
    return decoder_head_a(w, &cur.X, e->B, e->H, e->D, e->h_init, &cur.tp, drop, e->step0, ha, ep.stream);
}

// (3) Gate-space rows (include/sf_hip.h: sf_gate_rows_build), together with the projected chain only: launch (2) of step t
// leaves the chosen action's row in gate space in one of two [B, 4H] buffers carved off the FRONT of the workspace (the
// ticket region at its end keeps its address), step t + 1 runs its gate product over [f | h0] and its cell adds the row.
// Decided once, here, before the first launch; a step whose chain declines leaves `wrote` false and the step behind
// it runs the full product on the raw row, which every chain still writes.
// The attended half's table (sf_gate_rows_attended_build) adds two more rows `xg_f` beside them, under the same capacity
// rule, where the partials sit in launch (1) and take rows of 4H + LOC floats.
struct GateCarve {
    float* xg_buf[2] = {nullptr, nullptr};      // null: the full gate product in every step
    sf_gate_rows gr{};
    float* xgf_buf[2] = {nullptr, nullptr};     // null: the attended feature stays a raw row
    const float* gf = nullptr;
    float* xgh_buf[2] = {nullptr, nullptr};     // null: every cell forms h0 W_hh^T itself
};
GateCarve episode_gate_rows(const EpisodeFwd& ep, Arena& ar) {
    const sf_follower_episode* e = ep.e;
    const sf_decoder_w* w = ep.w;
    const sf_dropout* drop = ep.drop;
    const TextFold* tf = ep.tf;
    const sf_nav_io* nav0 = ep.nav0;
    const CandSrc& us0 = ep.us0;
    const PanoSrc& x0 = ep.x0;
    const Arena& whole = ar;
    GateCarve c;
    sf_gate_rows& gr = c.gr;
    const int F = us0.IMG + us0.LOC;
    const size_t row = ((size_t)e->B * 4 * e->H + 63) & ~(size_t)63;
    ProjTables pt;
    const void* packed[2];
    if (tf && !nav0 && !drop && e->S > 1 && e->B <= VIS_SPLIT_MAX_B && !us0.dense && !us0.half &&
        gate_rows_lookup(us0.table, &gr) && gr.key_w == w->lstm.w_ih && gr.H == e->H && gr.V == us0.V &&
        gr.IMG == us0.IMG && gr.LOC == us0.LOC && e->H % 4 == 0 && F % 4 == 0 && 2 * F + e->H > 1024 &&
        projected_for(w, us0, &x0, e->B, e->H, e->L, &pt) && !bf16_packed(w->lstm.w_ih, w->lstm.w_hh, packed) &&
        whole.tk && 2 * row <= whole.cap / 8) {
        c.xg_buf[0] = ar.base;
        c.xg_buf[1] = c.xg_buf[0] + row;
        ar.base = c.xg_buf[1] + row;
        ar.cap -= 2 * row;
        sf_gate_rows_attended ga{};
        if (gate_rows_attended_lookup(us0.table, &ga) && ga.key_w == gr.key_w && ga.H == gr.H && ga.V == gr.V &&
            ga.IMG == gr.IMG && ga.LOC == gr.LOC && !g_proj_partials_late && x0.IMG == us0.IMG && x0.LOC == us0.LOC &&
            proj_partials_supported(x0.IMG, x0.LOC) && proj_partials_supported(4 * e->H, x0.LOC) &&
            short_gate_fused(x0.LOC, e->H) && 4 * row <= whole.cap / 8) {
            c.gf = ga.gf;
            c.xgf_buf[0] = ar.base;
            c.xgf_buf[1] = c.xgf_buf[0] + row;
            ar.base = c.xgf_buf[1] + row;
            ar.cap -= 2 * row;
            // the recurrent half's rows (sf_gate_rows_recurrent_use) behind them, under the rule as the checks above apply
            // it: `whole` IS `ar`, so the six rows must fit an eighth of what is LEFT once the four rows above are carved
            // (52 rows <= the capacity this function was handed; the four-row check is 34 rows, the two-row check 16).  A
            // workspace too small for six keeps the four, and the episode runs what it ran without this row: with the
            // default 64 MB workspace at H = 512 that is B > 157 or a little below (tests/test_gpu_recurrent_row.py: B = 160)
            if (gate_rows_recurrent_on() && recurrent_row_cell(x0.LOC, e->H) && 6 * row <= whole.cap / 8) {
                c.xgh_buf[0] = ar.base;
                c.xgh_buf[1] = c.xgh_buf[0] + row;
                ar.base = c.xgh_buf[1] + row;
                ar.cap -= 2 * row;
            }
        }
    }
    return c;
}

// (4) the step loop.  A device-resident environment (sf_nav_io of step 0 in glue.nav; state buffers stacked
// [S + 1][...]): the panorama of step t + 1 is only known once the glue of step t has chosen its action and stepped the
// environment (inside the scoring + glue launch), so its attention cannot ride beside tail(t); its QUERY can
// (tape_next without X_next), and the attention follows as its own launch -- the schedule the host loop of
// FollowerEngine.rollout issues call by call, here without host work between the launches.
int episode_steps(const EpisodeFwd& ep, const GateCarve& c, Arena ar) {
    const sf_follower_episode* e = ep.e;
    const sf_decoder_w* w = ep.w;
    const sf_dropout* drop = ep.drop;
    const TextFold* tf = ep.tf;
    const sf_nav_io* nav0 = ep.nav0;
    const sf_gate_rows& gr = c.gr;
    float* const* xg_buf = c.xg_buf;
    const hipStream_t st = S(ep.stream);
    StepView cur = ep.cur;
    const float *xg_in = nullptr, *xg_f_in = nullptr, *xg_h_in = nullptr;
    for (int t = 0; t < e->S; ++t) {
        const bool more = t + 1 < e->S;
        StepView nxt = more ? step_view(e, t + 1) : cur;
        const sf_nav_io nv = nav0 ? nav_view(nav0, e, t) : sf_nav_io{};
        if (nav0) cur.glue.nav = &nv;
        const StepState in = state_in(e, t);
        GateStep gs{xg_in, GateRows{gr.gu, gr.gl, more ? xg_buf[t & 1] : nullptr, c.gf, more ? c.xgf_buf[t & 1] : nullptr,
                                    more ? c.xgh_buf[t & 1] : nullptr},
                    false, xg_f_in, false, xg_h_in};
        TRY(decoder_tail_i(w, &cur.U, e->B, e->H, e->D, e->L, nullptr, in.h, in.c, e->ctx, e->ctx_mask,
                           nullptr, &cur.tp, &cur.glue, drop, e->step0 + t, more && !nav0 ? &nxt.X : nullptr,
                           more ? &nxt.tp : nullptr, ar, st, tf, xg_buf[0] ? &gs : nullptr));
        xg_in = gs.wrote ? gs.rows.xg_next : nullptr;
        xg_f_in = gs.wrote && gs.wrote_f ? gs.rows.xg_f : nullptr;
        xg_h_in = xg_f_in && gs.wrote_h ? gs.rows.xg_h : nullptr;
        if (nav0 && more) TRY(attend_i(&nxt.X, e->B, &nxt.tp, drop, e->step0 + t + 1, ar, st));
        cur = nxt;
    }
    return SF_OK;
}

}  // namespace

extern "C" {

int sf_attn_decoder_head_fwd(const sf_decoder_w* w, const sf_pano* X, int B, int H, int D,
                             const float* h0, const sf_decoder_tape* tp, const sf_dropout* drop,
                             uint32_t step_id, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    return decoder_head_a(w, X, B, H, D, h0, tp, drop, step_id, arena(ws, ws_bytes), stream);
}

int sf_attn_decoder_attend_fwd(const sf_pano* X, int B, const sf_decoder_tape* tp, const sf_dropout* drop,
                               uint32_t step_id, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    return attend_i(X, B, tp, drop, step_id, arena(ws, ws_bytes), S(stream));
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
                          step_id, X_next, tn, arena(ws, ws_bytes), S(stream));
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
                          nullptr, arena(ws, ws_bytes), S(stream));
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

int sf_follower_episode_fwd(const sf_decoder_w* w, const sf_follower_episode* e, void* ws,
                            size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && e && e->S > 0 && e->B > 0 && e->h_init && e->c_init && e->ctx && e->tape.xin &&
                 e->tape.h1 && e->tape.c1 && e->glue.target && e->glue.ended);
    EpisodeFwd ep{w, e, e->drop.p > 0.f ? &e->drop : nullptr, e->glue.nav, step_view(e, 0)};
    ep.x0 = pano(&ep.cur.X);
    ep.us0 = cands(&ep.cur.U);
    ep.fold = TextFold{e->ctx_q, e->ctx_o};
    ep.tf = nullptr;
    ep.stream = stream;
    Arena ar = arena(ws, ws_bytes);
    TRY(episode_text_fold(ep, ar));
    TRY(episode_head(ep, ar));
    if (ep.nav0) SF_CHECK_ARG(w->visual.w_v_t);
    const GateCarve carve = episode_gate_rows(ep, ar);
    return episode_steps(ep, carve, ar);
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

}  // extern "C"
