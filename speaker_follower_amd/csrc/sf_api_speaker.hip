// The speaker: its path encoder (a8), its decoder step (a9), the word loop as one persistent launch, step by step with
// a tape, and teacher-forced; its glue and loss.  Host sequencing only (sf_api_util.h).
#include "sf_api_util.h"

using namespace sf;

namespace {

// row stride of the vocabulary logits: columns vocab..ldv-1 are padding, never read by the glue
inline int spk_ldv(int vocab) { return (vocab + 3) & ~3; }

// d h~ = dlogit W_out (dlogit [B,ldv] with zero padding columns): K-contiguous through decoder2action^T when the host
// keeps it (sf_spk_decoder_w.w_out_t [H,ldv]), else the strided NN kernel
int spk_dlogit_to_dht(const sf_spk_decoder_w* w, const float* dlogit, int ldv, int B, int H, int vocab, float* dht,
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

// ---- a8 SpeakerEncoderLSTM.forward (model.py:437-457), all path steps in one call -------------------------------------
int speaker_encoder_fwd_i(const sf_visual_fold64* fold64, const sf_visual_w* vw, const sf_lstm_w* lw, const float* w_e2d, const float* b_e2d,
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

// ---- the speaker's word loop with its tape, one call each way (speaker.py:158-197 and its backward) ------------------
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

extern "C" {

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
    const int ldv = spk_ldv(vocab);
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
    // cq = ctx W_in, cw = ctx W_c^T with W_c = linear_out[:, :H]
    TRY(context_fold(ctx, w->attn.w_in_t, w->attn.w_out, B * Tp, H, cq, cw, ar, st));
    return speaker_persistent(w->lstm.w_hh, w->lstm.b_ih, w->lstm.b_hh, w->xw_table, w->attn.w_out, 2 * H, w->w_out,
                              w->b_out, vocab, spk_ldv(vocab), cq, cw, ctx_mask, h_init, c_init, targets, feedback, pad_idx,
                              eos_idx, B, H, Tp, n_steps, words, step_scores, nll_term, live, logits, alpha, h1_tape,
                              c1_tape, ended, xchg, ar.tickets() + PERSIST_TICKET, st, sample);
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
    const int ldv = spk_ldv(vocab);
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

int sf_speaker_words_fwd(const sf_spk_decoder_w* w, int B, int E, int H, int Tp, int vocab, int S, int feedback,
                         int pad_idx, int eos_idx, const int64_t* targets, const float* h_init, const float* c_init,
                         const float* ctx, const uint8_t* ctx_mask, int64_t* words, uint8_t* ended, float* step_scores,
                         float* nll_term, float* live, const sf_spk_decoder_tape* tape0, const sf_dropout* drop,
                         uint32_t step0, const sf_sample* sample, void* ws, size_t ws_bytes, sf_stream stream) {
    SF_ENTER();
    SF_CHECK_ARG(w && tape0 && tape0->h1 && tape0->c1 && tape0->logit && targets && h_init && c_init && ctx && words &&
                 ended && step_scores && nll_term && live && B > 0 && S > 0 && (feedback != 2 || sample));
    const int ldv = spk_ldv(vocab);
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
    const int ldv = spk_ldv(vocab);
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
    const int M = S * B, ldv = spk_ldv(vocab);
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
    const int M = S * B, ldv = spk_ldv(vocab);
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

}  // extern "C"
