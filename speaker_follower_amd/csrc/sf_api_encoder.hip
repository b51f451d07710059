// The follower's instruction encoder (a5), one direction or two, forward and backward: host sequencing only
// (sf_api_util.h).
#include "sf_api_util.h"

using namespace sf;

namespace {
// ---- a5 bidirectional EncoderLSTM (model.py:47-66, 81-104 with bidirectional=True) -------------------------------
EncDir enc_dir(const sf_encoder_w* w, const sf_encoder_tape* tp) {
    return EncDir{w->lstm.w_hh, w->lstm.b_ih, w->lstm.b_hh, w->xw_table, tp->gates, tp->hs, tp->cs, tp->xg};
}
bool bi_persistent(const sf_encoder_w* f, const sf_encoder_w* r, int B, int H, int T) {
    return f->xw_table && r->xw_table && !(f->flags & SF_ENC_PER_STEP) && encoder_bi_persistent_supported(B, H, T);
}
// a nested entry-point call on what is left of the arena (the ticket region stays where it is)
inline size_t nested_bytes(const Arena& a) { return (a.rest_n() + SYNC_WORDS) * 4; }
}  // namespace

extern "C" {

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

}  // extern "C"
