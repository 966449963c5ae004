// The backward launch sequence: one encoder application, the sample-local query pass, and the whole step's backward with its weight-gradient
// batches, partial-slab bookkeeping and the two gradient reductions.  A dry run of it (Ctx::dry) lays out the partial arena of a training plan.
#include "host.hpp"

namespace vsl {

namespace {

// the loss launch of vsl_io.fused_loss on the current stream (run_backward decides where: in front of the heads' backward when they read the seeds
// from memory, at the end of the main stream's work when they compute them)
void loss_on_side(Ctx& c) {
    const vsl_loss_io* fl = c.pend_loss;
    if (!fl || c.dry) return;
    c.pend_loss = nullptr;
    const vsl_io* io = c.io;
    LAUNCH("loss", launch_loss(io->start_logits, io->end_logits, io->h_score, fl->start_labels, fl->end_labels, fl->h_labels, io->v_mask, io->B, io->T,
                               fl->inv_batch, fl->mask_sum, fl->w_loc, fl->w_highlight, c.W(c.p->loss_scratch), fl->losses, fl->d_start_logits,
                               fl->d_end_logits, fl->d_h_score, c.s, c.h->loss_counter));
}
// Every cross-stream ordering point (event record on the producer + wait on the consumer) leaves a ~6-7 us bubble in the
// producer stream (rocprofv3 timeline), so weight-gradient batches -- nothing waits for them before the final reduction --
// are collected while `defer_w` is set and go to the side stream behind ONE event.
void wgrad_async(Ctx& c, hipStream_t sw, const WgradBatch& wb) {
    if (c.defer_w) { c.pend.push_back(wb); return; }
    hipStream_t keep = c.s;
    c.order(keep, sw);
    c.s = sw;
    LAUNCH("wgrad", launch_wgrad(wb, c.s));
    c.s = keep;
}
void wgrad_flush(Ctx& c, hipStream_t sw) {
    if (c.pend.empty()) return;
    hipStream_t keep = c.s;
    c.order(keep, sw);
    c.s = sw;
    for (const WgradBatch& wb : c.pend) LAUNCH("wgrad", launch_wgrad(wb, c.s));
    c.s = keep;
    c.pend.clear();
}

WgradJob wjob() { WgradJob j; memset(&j, 0, sizeof j); return j; }

// The out_layer job and the fused q / k / v job of one encoder application, appended to `wb`; their partial slabs are allocated here, in this
// order (the sequence of slab / reg / part_alloc calls fixes the arena layout and the order in which k_reduce adds the sources)
void attn_wgrad_jobs(Ctx& c, const EncP& P, const EncWs& w, const EncTmp& t, WgradBatch& wb) {
    const Plan& p = *c.p;
    const int R = w.R, nchunk = (R + WG_ROWS - 1) / WG_ROWS;
    {
        WgradJob j = wjob();
        j.G[0] = c.dry ? nullptr : c.W(t.go); j.nG = 1; j.A[0] = c.dry ? nullptr : c.W(w.h2); j.nA = 1; j.K = D; j.R = R;
        j.out = c.slab(P.ow, D * D, nchunk);
        j.out_bias[0] = c.slab(P.ob, D, nchunk);
        wb.j[wb.n++] = j;
    }
    {
        WgradJob j = wjob();
        if (!c.dry) { j.G[0] = c.W(t.dq); j.G[1] = c.W(t.dk); j.G[2] = c.W(t.dv); j.A[0] = c.W(w.h1); }
        j.nG = 3; j.nA = 1; j.K = D; j.R = R;
        const int64_t o = c.part_alloc((int64_t)nchunk * 3 * D * D);
        c.reg(P.qw, D * D, p.partial + o, nchunk, 3 * D * D);
        c.reg(P.kw, D * D, p.partial + o + D * D, nchunk, 3 * D * D);
        c.reg(P.vw, D * D, p.partial + o + 2 * D * D, nchunk, 3 * D * D);
        j.out = c.part_ptr(o);
        j.out_bias[0] = c.slab(P.qb, D, nchunk);
        j.out_bias[1] = c.slab(P.kb, D, nchunk);
        j.out_bias[2] = c.slab(P.vb, D, nchunk);
        wb.j[wb.n++] = j;
    }
}

// the four pointwise-conv jobs of one encoder application, appended to `wb`, in chunks of Ctx::pw_rows rows (0 = WG_ROWS)
void pointwise_wgrad_jobs(Ctx& c, const EncP& P, const EncWs& w, const EncTmp& t, WgradBatch& wb) {
    for (int i = 0; i < 4; ++i) {
        WgradJob j = wjob();
        if (!c.dry) { j.G[0] = c.W(t.gz[i]); j.A[0] = c.W(w.u[i]); }
        j.nG = 1; j.nA = 1; j.K = D; j.R = w.R;
        j.rows = c.pw_rows;
        const int nch_pw = wgrad_chunks(w.R, wgrad_rows(j));
        j.out = c.slab(P.pw[i], D * D, nch_pw);
        j.out_bias[0] = c.slab(P.pwb[i], D, nch_pw);
        wb.j[wb.n++] = j;
    }
}

// the attention-output backward of encoder application `app` (its LayerNorm-2 partial slabs are allocated here: call once per application)
AttnOutBwdArgs attn_out_bwd_args(Ctx& c, const EncP& P, const EncPk& K, const EncWs& w, const float* dy, const float* dy2, int app) {
    const Plan& p = *c.p;
    const EncTmp& t = p.tmp[app];
    const int ntiles = (w.R + TILE_M - 1) / TILE_M;
    float* p_ln2g = c.slab(P.ln2g, D, ntiles);
    float* p_ln2b = c.slab(P.ln2b, D, ntiles);
    AttnOutBwdArgs a;
    memset(&a, 0, sizeof a);
    if (!c.dry) a = AttnOutBwdArgs{dy, dy2, c.W(w.r), c.P(P.ln2g), c.PK(K.o_t), c.W(t.go), c.W(t.dr), p_ln2g, p_ln2b, c.drop(app * 16 + 7), c.drop(app * 16 + 8)};
    return a;
}
// backward of one FeatureEncoder application: dy = grad wrt its output; writes grad wrt its input (dx0_out)
// attn_out_done: the attention-output backward of this application already ran (fused into the span heads' kernel: run_backward)
// tail_ao / tail_cq: what the conv block's backward workgroups go on with on their tile of dx0 (CbBwdArgs::tail; the caller has checked
// convblock_bwd_hosts_tail and skips that launch)
struct LinTail { const uint16_t* WT3; float* dA; int K, Kc; };     // CbBwdArgs::tail == 3
void enc_bwd(Ctx& c, const EncP& P, const EncPk& K, const EncWs& w, const float* dy, const float* dy2, int64_t dx0_off,
             const float* mask, int Bn, int app, hipStream_t sw, WgradBatch* defer_pw = nullptr, bool attn_out_done = false,
             const AttnOutBwdArgs* tail_ao = nullptr, const CqcatBwdArgs* tail_cq = nullptr, const LinTail* tail_lin = nullptr) {
    // sw: stream of the early (out_layer / q,k,v) weight gradients.  The pointwise-conv batch goes to `sw` too unless the
    // caller asks for it back (defer_pw) to launch it on its own stream WITHOUT a cross-stream wait (each costs ~16 us).
    float* dx0_out = c.dry ? nullptr : c.W(dx0_off);
    const Plan& p = *c.p;
    const EncTmp& t = p.tmp[app];
    const int R = w.R, L = w.L, H = c.h->cfg.num_heads;
    const int ntiles = (R + TILE_M - 1) / TILE_M;
    if (!attn_out_done) {
        const AttnOutBwdArgs ao = attn_out_bwd_args(c, P, K, w, dy, dy2, app);
        LAUNCH("attn_out_bwd", launch_attn_out_bwd(ao.dy, ao.dy2, ao.r_in, ao.ln_g, ao.WTpack, ao.g_o, ao.dr, ao.p_lng, ao.p_lnb, R, ao.d4, ao.d5, c.s));
    }
    // every head count, every L: key-major dK / dV; dQ as attn_dq_slabs(L) slabs (L > ATTN_SLAB_MAX_L: query-major into slab 0, kernels_attn.hip)
    LAUNCH("attn_bwd", launch_attn_bwd(AttnArgs{c.W(w.q), c.W(w.k), c.W(w.v), mask, c.W(w.att), c.W(w.lse), c.W(t.dr), c.W(t.dq), c.W(t.dk), c.W(t.dv),
                                                Bn, L, H, 0, c.drop(app * 16 + 5), c.drop(app * 16 + 6)}, c.s));
    // whole tiles / sample tiles (and one dQ slab): the conv block's backward kernel computes its own incoming gradient from dq / dk / dv (CbBwdArgs::qk).
    // The gate stays on the key-major slab count: L > 256 never fuses, the one-slab dQ of L > ATTN_SLAB_MAX_L included (k_qkv_bwd adds nothing there)
    static const bool fuse_on = !(getenv("VSL_QKV_FUSED") && getenv("VSL_QKV_FUSED")[0] == '0');
    const bool fuse_qkv = fuse_on && convblock_bwd_hosts_qkv(R, L) && attn_bwd_dq_slabs(L) == 1;
    const int nsl1 = fuse_qkv ? convblock_slabs(R, L) : ntiles;
    float* p_ln1g = c.slab(P.ln1g, D, nsl1);
    float* p_ln1b = c.slab(P.ln1b, D, nsl1);
    if (!fuse_qkv)
        LAUNCH("qkv_bwd", launch_qkv_bwd(c.W(t.dq), c.W(t.dk), c.W(t.dv), c.W(w.y[3]), c.W(t.dr), c.P(P.ln1g), reinterpret_cast<const uint16_t*>(c.PK(K.qkv_t3)),
                              c.W(t.ga), p_ln1g, p_ln1b, R, c.drop(app * 16 + 4), c.s, attn_dq_slabs(L)));
    {   // out_layer + fused q/k/v weight gradients: every input exists now -> side stream, beside the conv chain
        WgradBatch wb;
        memset(&wb, 0, sizeof wb);
        attn_wgrad_jobs(c, P, w, t, wb);
        wgrad_async(c, sw, wb);
    }
    float* g = c.dry ? nullptr : c.W(t.ga);
    {
        // the four layers in ONE launch (kernels_enc.hip: 12-row recomputed halo); slab order = the per-layer chain's
        CbBwdArgs a;
        memset(&a, 0, sizeof a);
        const int nsl = convblock_slabs(R, L);
        for (int i = 3; i >= 0; --i) {
            a.p_lng[i] = c.slab(P.lng[i], D, nsl);
            a.p_lnb[i] = c.slab(P.lnb[i], D, nsl);
            a.p_dw[i] = c.slab(P.dw[i], D * DWK, nsl);
        }
        if (tail_ao) { a.tail = 1; a.tail_ao = *tail_ao; }
        if (tail_cq) { a.tail = 2; a.tail_cq = *tail_cq; }
        if (tail_lin) { a.tail = 3; a.tail_lin_WT3 = tail_lin->WT3; a.tail_lin_dA = tail_lin->dA; a.tail_lin_K = tail_lin->K; a.tail_lin_Kc = tail_lin->Kc; }
        if (fuse_qkv) {
            a.qkv = 1;
            if (!c.dry) a.qk = QkvBwdFuse{c.W(t.dq), c.W(t.dk), c.W(t.dv), c.W(w.y[3]), c.W(t.dr), c.P(P.ln1g), reinterpret_cast<const uint16_t*>(c.PK(K.qkv_t3)),
                                          p_ln1g, p_ln1b, c.drop(app * 16 + 4)};
        }
        if (!c.dry) {
            a.dy = g; a.dx0 = dx0_out; a.R = R; a.L = L;
            for (int i = 0; i < 4; ++i) {
                a.x[i] = i > 0 ? c.W(w.y[i - 1]) : c.W(w.x0);
                a.relu_mask[i] = reinterpret_cast<const uint32_t*>(c.W(w.mask[i]));
                a.ln_g[i] = c.P(P.lng[i]); a.ln_b[i] = c.P(P.lnb[i]); a.dw_w[i] = c.P(P.dw[i]);
                a.dp[i] = c.drop(app * 16 + i); a.gz[i] = c.W(t.gz[i]);
                a.WT3[i] = reinterpret_cast<const uint16_t*>(c.PK(K.pw_t3[i]));
            }
        }
        LAUNCH("convblock_bwd", launch_convblock_bwd(a, c.s));
    }
    // pointwise-conv weight gradients (inputs complete only now); Wo / QKV were launched right after qkv_bwd
    {
        WgradBatch wb;
        memset(&wb, 0, sizeof wb);
        pointwise_wgrad_jobs(c, P, w, t, wb);
        if (defer_pw) *defer_pw = wb;
        else wgrad_async(c, sw, wb);
    }
    // positional table (:202): dpos[t] = sum_b dx0[b, t] -- the per-sample rows of dx0 ARE the partial slabs
    c.reg(P.pos, c.h->cfg.max_pos_len * D, dx0_off, Bn, L * D, 0, 0, L * D);
}

// the query pass' backward as ONE sample-local launch (kernels_query.hip: k_query_bwd) + the weight-gradient jobs that read what it leaves:
// out_layer, fused q/k/v, the four pointwise convs (the Embedding linear's job is the caller's: it also owns dqf / E)
void query_bwd(Ctx& c, const float* dy, int64_t dx0_off, WgradBatch& jobs) {
    const vsl_config& cf = c.h->cfg;
    const ModelPk& MK = c.h->K;
    const EncP& P = c.h->P.fe;
    const EncPk& K = c.h->K.fe;
    const Plan& p = *c.p;
    const EncWs& w = p.qe;
    const EncTmp& t = p.tmp[1];
    const int B = p.B, Lq = p.Lq, app = 1;
    QueryBwdArgs a;
    memset(&a, 0, sizeof a);
    a.p_ln2g = c.slab(P.ln2g, D, B); a.p_ln2b = c.slab(P.ln2b, D, B);
    a.p_ln1g = c.slab(P.ln1g, D, B); a.p_ln1b = c.slab(P.ln1b, D, B);
    for (int i = 3; i >= 0; --i) {
        a.p_lng[i] = c.slab(P.lng[i], D, B);
        a.p_lnb[i] = c.slab(P.lnb[i], D, B);
        a.p_dw[i] = c.slab(P.dw[i], D * DWK, B);
    }
    if (!c.dry) {
        a.dout = dy; a.r = c.W(w.r); a.ln2_g = c.P(P.ln2g); a.WoT3 = reinterpret_cast<const uint16_t*>(c.PK(K.o_t3)); a.go = c.W(t.go);
        a.d2 = c.drop(app * 16 + 5); a.d3 = c.drop(app * 16 + 6); a.d4 = c.drop(app * 16 + 7); a.d5 = c.drop(app * 16 + 8);
        a.q = c.W(w.q); a.k = c.W(w.k); a.v = c.W(w.v); a.att = c.W(w.att); a.lse = c.W(w.lse); a.mask = c.io->q_mask;
        a.dq = c.W(t.dq); a.dk = c.W(t.dk); a.dv = c.W(t.dv);
        a.WqkvT3 = reinterpret_cast<const uint16_t*>(c.PK(K.qkv_t3)); a.y3 = c.W(w.y[3]); a.ln1_g = c.P(P.ln1g); a.d1 = c.drop(app * 16 + 4);
        for (int i = 0; i < 4; ++i) {
            a.WT3[i] = reinterpret_cast<const uint16_t*>(c.PK(K.pw_t3[i]));
            a.x[i] = i > 0 ? c.W(w.y[i - 1]) : c.W(w.x0);
            a.relu_mask[i] = reinterpret_cast<const uint32_t*>(c.W(w.mask[i]));
            a.ln_g[i] = c.P(P.lng[i]); a.ln_b[i] = c.P(P.lnb[i]); a.dw_w[i] = c.P(P.dw[i]);
            a.dp[i] = c.drop(app * 16 + i); a.gz[i] = c.W(t.gz[i]);
        }
        a.dx0 = c.W(dx0_off);
        a.WembT3 = reinterpret_cast<const uint16_t*>(c.PK(MK.emb_t3)); a.dE = c.W(p.dE);
        a.EW = cf.word_dim + 100; a.EWc = MK.emb_t3_cols; a.L = Lq; a.b_off = 0;
    }
    LAUNCH("query_bwd", launch_query_bwd(a, B, c.s));
    attn_wgrad_jobs(c, P, w, t, jobs);
    pointwise_wgrad_jobs(c, P, w, t, jobs);       // (Ctx::pw_rows is 0 here: WG_ROWS chunks)
    c.reg(P.pos, cf.max_pos_len * D, dx0_off, B, Lq * D, 0, 0, Lq * D);     // positional table (:202): the per-sample rows of dx0 are the partial slabs
}

}  // namespace

void run_backward(Ctx& c) {
    const vsl_config& cf = c.h->cfg;
    const ModelP& P = c.h->P;
    const ModelPk& K = c.h->K;
    const Plan& p = *c.p;
    const int B = p.B, T = p.T, Lq = p.Lq, R = B * T, Rq = B * Lq;
    const int ntiles = (R + TILE_M - 1) / TILE_M, nchunk = (R + WG_ROWS - 1) / WG_ROWS, nchunk_q = (Rq + WG_ROWS - 1) / WG_ROWS;
    // a step through a shared encoding (plan TrainShared): the video half -- encoder application 0 and VisualProjection -- runs on Nv T rows
    const bool shared = p.kind == PlanKind::TrainShared;
    const int Nv = p.NV(), Rv = Nv * T;
    const vsl_io* io = c.io;
    // streams: `main` carries the dependent dX chain; sw = every weight-gradient GEMM (they only feed the final
    // reduction); sq = the query-side chain (query encoder pass + embedding stack) once CQAttention's backward is done
    hipStream_t sw = c.dry ? nullptr : c.side(1), sq = c.dry ? nullptr : c.side(0);
    auto on_stream = [&](hipStream_t st, auto&& fn) { hipStream_t keep = c.s; c.order(keep, st); c.s = st; fn(); c.s = keep; };
    c.defer_w = !c.dry && cf.predictor == 1;
    bool hosted = false;                    // transformer head on whole tiles: two launches ride inside the conv block's backward kernels (below)
    float *p_hlw = nullptr, *p_hlb = nullptr;
    CqcatBwdArgs cqa;
    // ---- span heads
    HeadBwdArgs hs, he;
    memset(&hs, 0, sizeof hs);
    memset(&he, 0, sizeof he);
    const bool rnn = cf.predictor == 0;
    // vsl_io.fused_loss: the loss is part of this call.  Whole tiles + the caller's mask sum: k_loss_fused goes to the weight-gradient stream (nothing
    // on the dependent chain reads what it writes) and the consumers of the seeds -- the span heads' backward, the highlight layer's -- compute
    // them from the logits themselves.  Otherwise the loss launches first, on the caller's stream, and the seeds are read as they always were.
    const vsl_loss_io* fl = c.dry ? nullptr : io->fused_loss;
    const float *seed_s = nullptr, *seed_e = nullptr, *seed_h = nullptr;
    bool seeds_inline = false;
    HlSeed hlseed{nullptr, nullptr, 0.f, 0.f};
    if (!c.dry) {
        seed_s = fl ? fl->d_start_logits : io->d_start_logits; seed_e = fl ? fl->d_end_logits : io->d_end_logits; seed_h = fl ? fl->d_h_score : io->d_h_score;
        if (fl) {
            static const bool inline_on = !(getenv("VSL_LOSS_INLINE") && getenv("VSL_LOSS_INLINE")[0] == '0');
            seeds_inline = inline_on && T >= TILE_M && fl->mask_sum > 0.f && c.h->loss_counter != nullptr;       // (T >= 32: a row tile touches at most two samples)
            c.pend_loss = fl;
            if (!seeds_inline) loss_on_side(c);            // (here and now, on the caller's stream: the seeds are read from memory)
            else hlseed = HlSeed{fl->h_labels, io->v_mask, fl->w_highlight, fl->mask_sum};
        }
        hs = HeadBwdArgs{seed_s, c.W(p.hid_s), c.W(p.p1.out), rnn ? nullptr : c.P(P.sln_g), c.PK(K.s0_t), c.P(P.s1w), c.W(p.gz_s),
                         c.W(p.dfeat_s), c.W(p.dxh_s), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0};
        he = HeadBwdArgs{seed_e, c.W(p.hid_e), c.W(p.p2.out), rnn ? nullptr : c.P(P.eln_g), c.PK(K.e0_t), c.P(P.e1w), c.W(p.gz_e),
                         c.W(p.dfeat_e), c.W(p.dxh_e), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0};
        if (seeds_inline) {
            hs.logits = io->start_logits; hs.label = fl->start_labels; hs.cs = fl->w_loc * fl->inv_batch; hs.T = T;
            he.logits = io->end_logits; he.label = fl->end_labels; he.cs = fl->w_loc * fl->inv_batch; he.T = T;
        }
    }
    hs.p_b0 = c.slab(P.s0b, D, ntiles); hs.p_w1 = c.slab(P.s1w, D, ntiles); hs.p_b1 = c.slab(P.s1b, 1, ntiles);
    he.p_b0 = c.slab(P.e0b, D, ntiles); he.p_w1 = c.slab(P.e1w, D, ntiles); he.p_b1 = c.slab(P.e1b, 1, ntiles);
    if (!rnn) {
        hs.p_lng = c.slab(P.sln_g, D, ntiles); hs.p_lnb = c.slab(P.sln_b, D, ntiles);
        he.p_lng = c.slab(P.eln_g, D, ntiles); he.p_lnb = c.slab(P.eln_b, D, ntiles);
    }
    // transformer head: the end head's workgroups run the attention-output backward of the second predictor pass on their own tile of dfeat_e
    AttnOutBwdArgs ao2;
    if (!rnn) ao2 = attn_out_bwd_args(c, P.pe, K.pe, p.p2, nullptr, nullptr, 3);
    LAUNCH("head_bwd", launch_head_bwd(hs, he, R, c.s, rnn ? nullptr : &ao2));
    {
        WgradBatch wb;
        memset(&wb, 0, sizeof wb);
        for (int e = 0; e < 2; ++e) {
            WgradJob j = wjob();
            if (!c.dry) { j.G[0] = c.W(e ? p.gz_e : p.gz_s); j.A[0] = rnn ? c.W(p.lstm[e].out) : c.W(e ? p.lnf_e : p.lnf_s); j.A[1] = c.W(p.gated); }
            j.nG = 1; j.nA = 2; j.K = 2 * D; j.R = R;
            j.out = c.slab(e ? P.e0w : P.s0w, D * 2 * D, nchunk);
            wb.j[wb.n++] = j;
        }
        wgrad_async(c, sw, wb);
    }
    if (rnn) {
        // ---- rnn head: BPTT through the end LSTM, then the start LSTM (whose output also feeds the start span block).
        //      Pipelined in time chunks like the forward (fuse_and_predict): the end LSTM walks the chunks backwards on the main
        //      stream; behind it the side stream turns the chunk's gate gradients into the start LSTM's incoming gradient
        //      (dx = dG W_ih, row-mapped GEMM) and runs the start LSTM over the same chunk.
        const std::vector<int> chunks = lstm_chunks(T);
        auto bwd = [&](int l, int t0, int t1) {
            const LstmWs& w = p.lstm[l];
            const float* d1 = c.dry ? nullptr : c.W(l ? p.dfeat_e : p.dfeat_s);
            const float* d2 = (c.dry || l) ? nullptr : c.W(p.g_s1);
            LAUNCH("lstm_bwd", launch_lstm_bwd(d1, d2, io->v_mask, c.W(w.gates), c.W(w.cseq), c.W(w.tseq), c.P(P.l_whh[l]), c.PK(K.l_hb[l]), c.W(w.dG),
                                               B, T, c.s, c.W(w.carry), t0, t1));
        };
        // dx = dG W_ih : (rows,512) x (512,128), K-streamed GEMM kernel of the visual projection, no dropout, zero bias
        auto dx = [&](int l, int t0, int t1) {
            const LstmWs& w = p.lstm[l];
            const bool all = t0 == 0 && t1 == T;
            LAUNCH("lstm_dx", launch_vproj_fwd3(c.W(w.dG), reinterpret_cast<const uint16_t*>(c.PK(K.l_t3[l])), c.PK(K.zero128), c.W(l ? p.g_s1 : p.g_gated),
                                               all ? R : B * (t1 - t0), 4 * D, Drop{0u, 0u, 1.f}, c.s, all ? 0 : t1 - t0, T, t0));
        };
        const bool piped = !c.dry && chunks.size() >= 2 && sq != c.s;
        if (!c.dry) {
            if (p.h_gran >= 0) {
                RnnBwdArgs a;
                memset(&a, 0, sizeof a);
                a.dout[0] = c.W(p.dfeat_s); a.dout[1] = c.W(p.dfeat_e); a.mask = io->v_mask; a.Wih1 = c.PK(K.l_ib);
                for (int l = 0; l < 2; ++l) {
                    const LstmWs& w = p.lstm[l];
                    a.gates[l] = c.W(w.gates); a.cseq[l] = c.W(w.cseq); a.tseq[l] = c.W(w.tseq); a.Whh[l] = c.PK(K.l_hb[l]); a.dG[l] = c.W(w.dG);
                }
                a.dg_gran = reinterpret_cast<unsigned long long*>(c.W(p.dg_gran)); a.dx_gran = reinterpret_cast<unsigned long long*>(c.W(p.dx_gran));
                long long gen = 0;
                a.epoch = rnn_epoch(&gen); a.B = B; a.T = T;
                rnn_granules_fresh(c, *c.p, gen);
                LAUNCH("rnn_bwd", launch_rnn_bwd(a, c.s));
                dx(0, 0, T);
            } else if (!piped) {
                bwd(1, 0, T); dx(1, 0, T); bwd(0, 0, T); dx(0, 0, T);
            } else {
                hipStream_t main_s = c.s;
                int t1 = T;
                hipStream_t sg = sw != main_s ? sw : sq;      // the dx GEMM of a chunk beside the start LSTM's previous chunk (see fuse_and_predict)
                for (int len : chunks) {
                    const int t0 = t1 - len;
                    bwd(1, t0, t1);
                    c.order(main_s, sg);
                    c.s = sg;
                    dx(1, t0, t1);
                    c.order(sg, sq);
                    c.s = sq;
                    bwd(0, t0, t1);
                    c.s = main_s;
                    t1 = t0;
                }
                c.order(sq, main_s);
                dx(0, 0, T);
            }
        }
        for (int l = 1; l >= 0; --l) {
            const LstmWs& w = p.lstm[l];
            // weight gradients: dW_ih = dG^T x, dW_hh = dG^T h_prev, db_ih = db_hh = column sums of dG (two gate pairs per job)
            WgradBatch wb;
            memset(&wb, 0, sizeof wb);
            for (int which = 0; which < 2; ++which) {                     // 0: W_ih (+ biases), 1: W_hh
                for (int half = 0; half < 2; ++half) {
                    WgradJob j = wjob();
                    if (!c.dry) {
                        j.G[0] = c.W(w.dG) + (2 * half) * D; j.G[1] = c.W(w.dG) + (2 * half + 1) * D;
                        j.A[0] = which ? c.W(w.hprev) : (l ? c.W(p.lstm[0].out) : c.W(p.gated));
                    }
                    j.nG = 2; j.nA = 1; j.K = D; j.R = R; j.ldg = 4 * D;
                    const int dst = (which ? P.l_whh[l] : P.l_wih[l]) + half * 2 * D * D;
                    j.out = c.slab(dst, 2 * D * D, nchunk);
                    if (which == 0) {
                        for (int g = 0; g < 2; ++g) {
                            const int64_t o = c.part_alloc((int64_t)nchunk * D);
                            c.reg(P.l_bih[l] + (2 * half + g) * D, D, p.partial + o, nchunk, D);
                            c.reg(P.l_bhh[l] + (2 * half + g) * D, D, p.partial + o, nchunk, D);
                            j.out_bias[g] = c.part_ptr(o);
                        }
                    }
                    wb.j[wb.n++] = j;
                }
            }
            on_stream(sw, [&] { LAUNCH("wgrad", launch_wgrad(wb, c.s)); });
        }
    } else {
    // ---- predictor encoder, second pass (input = output of the first pass), then first pass
    // tile-local continuations inside the conv block's backward kernel (whole tiles): pass 2's conv block goes on with pass 1's attention-output
    // backward (dy = its dx0 + the start head's LayerNorm path), pass 1's with the CQConcatenate backward (dg0 = its dx0)
    hosted = convblock_bwd_hosts_tail(R, T);
    AttnOutBwdArgs ao1;
    if (hosted) ao1 = attn_out_bwd_args(c, P.pe, K.pe, p.p1, nullptr, c.dry ? nullptr : c.W(p.dfeat_s), 2);
    enc_bwd(c, P.pe, K.pe, p.p2, c.dry ? nullptr : c.W(p.dfeat_e), nullptr, p.g_s1, c.dry ? nullptr : io->v_mask, B, 3, sw, nullptr, true,
            hosted ? &ao1 : nullptr);
    wgrad_flush(c, sw);   // span heads + pass-2 weight gradients: one ordering point
    // grad wrt the first pass' output = (input grad of the second pass) + (LayerNorm path of the start head)
    if (hosted) {
        p_hlw = c.slab(P.hl_w, D, ntiles);
        p_hlb = c.slab(P.hl_b, 1, ntiles);
        memset(&cqa, 0, sizeof cqa);
        if (!c.dry) cqa = CqcatBwdArgs{nullptr, c.W(p.dxh_s), c.W(p.dxh_e), seed_h, c.W(p.f2), io->h_score, c.P(P.hl_w), c.PK(K.cat1_t), c.W(p.df2), c.W(p.df1), p_hlw, p_hlb,
                                       hlseed.h_lab, hlseed.vmask, hlseed.w_hl, hlseed.mask_sum};
    }
    enc_bwd(c, P.pe, K.pe, p.p1, c.dry ? nullptr : c.W(p.g_s1), c.dry ? nullptr : c.W(p.dfeat_s), p.g_gated,
            c.dry ? nullptr : io->v_mask, B, 2, sw, nullptr, hosted, nullptr, hosted ? &cqa : nullptr);
    }
    // ---- gating + highlight + CQConcatenate
    if (!hosted) {
        p_hlw = c.slab(P.hl_w, D, ntiles);
        p_hlb = c.slab(P.hl_b, 1, ntiles);
        LAUNCH("cqcat_bwd", launch_cqcat_bwd(c.W(p.g_gated), c.W(p.dxh_s), c.W(p.dxh_e), seed_h, c.W(p.f2), io->h_score, c.P(P.hl_w),
                                c.PK(K.cat1_t), c.W(p.df2), c.W(p.df1), p_hlw, p_hlb, R, c.s, hlseed.h_lab ? &hlseed : nullptr));
    }
    {
        WgradBatch wb;
        memset(&wb, 0, sizeof wb);
        {   // first half of the (128, 256) CQConcatenate weight: destination rows are strided by 256
            WgradJob j = wjob();
            if (!c.dry) { j.G[0] = c.W(p.df2); j.A[0] = c.W(p.f1); }
            j.nG = 1; j.nA = 1; j.K = D; j.R = R;
            const int64_t o = c.part_alloc((int64_t)nchunk * D * D);
            c.reg(P.cat_w, D * D, p.partial + o, nchunk, D * D, D, 2 * D);
            j.out = c.part_ptr(o);
            wb.j[wb.n++] = j;
        }
        {   // cqa_linear (128, 512)
            WgradJob j = wjob();
            if (!c.dry) { j.G[0] = c.W(p.df1); j.Afull = c.W(p.cat); }
            j.nG = 1; j.nA = 0; j.K = 4 * D; j.R = R;
            j.out = c.slab(P.cqa_w, D * 4 * D, nchunk);
            j.out_bias[0] = c.slab(P.cqa_b, D, nchunk);
            wb.j[wb.n++] = j;
        }
        wgrad_async(c, sw, wb);
        wgrad_flush(c, sw);                 // pass-1 + fusion weight gradients: one ordering point
        c.defer_w = false;
    }
    // ---- CQAttention + WeightedPool / pooled-bias backward: four tile-parallel kernels (kernels_bwd.hip)
    CqBwdArgs q;
    {
        const int ntile = (T + TILE_M - 1) / TILE_M;
        memset(&q, 0, sizeof q);
        if (!c.dry) {
            q.df1 = c.W(p.df1); q.df2 = c.W(p.df2); q.C = c.W(p.ve.out); q.Qf = c.W(p.qe.out); q.Srow = c.W(p.Srow);
            q.Scol = c.W(p.Scol); q.M = c.W(p.M); q.alpha = c.W(p.alpha); q.pooled = c.W(p.pooled); q.WcqaT = c.PK(K.cqa_t);
            q.w4C = c.P(P.w4C); q.w4Q = c.P(P.w4Q); q.w4mlu = c.P(P.w4mlu); q.pool_w = c.P(P.pool_w); q.Wcat = c.P(P.cat_w);
            q.dC = c.W(p.dC); q.dQ = c.W(p.dQtot); q.dSr = c.W(p.dSr); q.dSs = c.W(p.dSs);
            q.P1 = c.W(p.cqP1); q.P2 = c.W(p.cqP2); q.P3 = c.W(p.cqP3); q.P4 = c.W(p.cqP4); q.P5 = c.W(p.cqP5);
        }
        if (shared && !c.dry) q.vidx = c.sh->video_index;        // C is the (Nv, T, 128) encoding; dC stays (B, T, 128)
        q.T = T; q.Lq = Lq; q.b_off = 0; q.dc = c.drop(SITE_CQ_C); q.dq = c.drop(SITE_CQ_Q);
        q.p_w4C = c.slab(P.w4C, D, B * ntile); q.p_w4mlu = c.slab(P.w4mlu, D, B * ntile);
        q.p_w4Q = c.slab(P.w4Q, D, B); q.p_pool = c.slab(P.pool_w, D, B); q.p_bcat = c.slab(P.cat_b, D, B);
        const int64_t o = c.part_alloc((int64_t)B * D * D);
        c.reg(P.cat_w + D, D * D, p.partial + o, B, D * D, D, 2 * D);          // second half of the (128, 256) weight
        q.p_W2 = c.part_ptr(o);
        LAUNCH("cq_bwd", launch_cq_bwd(q, B, c.s));
    }
    // early reduction (predictor / heads / CQ parameters): all their partials exist once the launches above are done
    // (the pooled-query parameters of k_cq_bwd_d belong to the late reduction: that kernel opens the query chain below).
    // ONE event for both consumers: the early reduction on sw and the fork of the query side onto sq
    c.order2(c.s, sw, sq);
    { hipStream_t keep = c.s; c.s = sw; LAUNCH("reduce", launch_reduce(c.ws, io->grads, p.segs_dev, p.blk2seg_dev, p.nblocks_early, p.sq_dev, c.s)); c.s = keep; }
    // data parallel: the predictor block of the gradient bucket is final now -- the caller's all-reduce of it can start (vslnet_hip.h)
    if (!c.dry && io->early_grads_event && cf.predictor == 1) (void)hipEventRecord((hipEvent_t)io->early_grads_event, sw);
    // from here the video side and the query side are independent; the longer one keeps the main stream
    hipStream_t main_s = c.s;
    const bool qlong = query_chain_is_longer(p);
    c.s = qlong ? sq : main_s;
    WgradBatch pw_video;
    memset(&pw_video, 0, sizeof pw_video);
    // The step's LAST weight-gradient batch (VisualProjection + the video pass' four pointwise gradients, sample-local query path) starts into an
    // empty chip: chunk rows that make it whole rounds of one-workgroup-per-CU chunks (Dv = 1024: 12 blocks x 32 chunks = 1.5 rounds -> 400 rows,
    // 252 workgroups; profiles/r06_notes.md section 8: -0.6 % against 256-row chunks).
    const int tail_rows = query_fused(c) ? wgrad_rows_whole_rounds(Rv, (cf.video_feature_dim + 127) / 128 + 4, c.h->cus) : WG_ROWS;
    c.pw_rows = tail_rows == WG_ROWS ? 0 : tail_rows;
    // shared encoding: dCv[n] = the sum of dC[b] over the queries of video n in ascending b (kernels_shared.hip; the CSR is the forward's), a
    // stand-alone launch at the head of the video chain
    if (shared) {
        const int* csr = c.dry ? nullptr : reinterpret_cast<const int*>(c.W(p.csr));
        LAUNCH("group_sum", launch_group_sum(c.W(p.dC), csr, csr + p.csr_members(), c.W(p.dCv), Nv, T, c.s));
    }
    enc_bwd(c, P.fe, K.fe, p.ve, c.dry ? nullptr : c.W(shared ? p.dCv : p.dC), nullptr, p.dvf, c.dry ? nullptr : c.video_mask(), Nv, 0, sw, &pw_video);
    c.pw_rows = 0;
    {   // tail of the video stream: VisualProjection + the video pass' pointwise weight gradients, back to back, no waits
        WgradBatch wb;
        memset(&wb, 0, sizeof wb);
        WgradJob j = wjob();
        j.rows = tail_rows == WG_ROWS ? 0 : tail_rows;
        const int nchunk = wgrad_chunks(Rv, tail_rows);     // (shadows the 256-row count: this job's slabs)
        if (!c.dry) {
            j.G[0] = c.W(p.dvf); j.Afull = io->video_features;
            if (io->video_features_bf16) { j.Afull = reinterpret_cast<const float*>(io->video_features_bf16); j.a_bf16 = 1; }
        }
        j.nG = 1; j.nA = 0; j.K = cf.video_feature_dim; j.R = Rv; j.drop_on_A = 1; j.dp = c.drop(SITE_VIS);
        j.out = c.slab(P.va_w, D * cf.video_feature_dim, nchunk);
        j.out_bias[0] = c.slab(P.va_b, D, nchunk);
        wb.j[wb.n++] = j;
        // sample-local query backward (kernels_query.hip): nothing on the video stream waits for the query chain any more -- the video pass'
        // pointwise weight gradients ride in THIS launch, the query side's own batch goes to the weight-gradient stream behind k_query_bwd.
        // (Measured and dropped: the video pass' pointwise batch on the weight-gradient stream instead, +3.5 %: profiles/r06_notes.md)
        if (query_fused(c)) { for (int i = 0; i < pw_video.n; ++i) wb.j[wb.n++] = pw_video.j[i]; }
        LAUNCH("wgrad", launch_wgrad(wb, c.s));
    }
    // ---- query pass, then the embedding stack (all on the other stream)
    c.s = qlong ? main_s : sq;
    LAUNCH("cq_bwd_d", launch_cq_bwd_query(q, B, c.s));     // dQ: only the query side consumes it
    WgradBatch pw_query;
    memset(&pw_query, 0, sizeof pw_query);
    const int EW = cf.word_dim + 100;
    // sample tiles (Lq <= 32): the query pass' conv-block backward goes on with the Embedding linear's data gradient on its rows of dx0
    const bool qfused = query_fused(c);
    const bool lin_hosted = qfused || (convblock_bwd_hosts_linear(Rq, Lq) && K.emb_t3_cols % 512 == 0);
    LinTail lt{nullptr, nullptr, EW, K.emb_t3_cols};
    if (lin_hosted && !c.dry) { lt.WT3 = reinterpret_cast<const uint16_t*>(c.PK(K.emb_t3)); lt.dA = c.W(p.dE); }
    if (qfused) query_bwd(c, c.dry ? nullptr : c.W(p.dQtot), p.dqf, pw_query);
    else
    enc_bwd(c, P.fe, K.fe, p.qe, c.dry ? nullptr : c.W(p.dQtot), nullptr, p.dqf, c.dry ? nullptr : io->q_mask, B, 1, sw, &pw_query, false, nullptr, nullptr,
            lin_hosted ? &lt : nullptr);
    {   // every remaining weight gradient (video + query pointwise convs, embedding linear) in ONE launch on the video
        // stream, beside the embedding backward that ends the query stream
        WgradBatch wb_tail = pw_video;
        if (qfused) wb_tail.n = 0;
        WgradJob j = wjob();
        if (!c.dry) { j.G[0] = c.W(p.dqf); j.Afull = c.W(p.E); }
        j.nG = 1; j.nA = 0; j.K = EW; j.R = Rq;
        j.out = c.slab(P.emb_w, D * EW, nchunk_q);
        j.out_bias[0] = c.slab(P.emb_b, D, nchunk_q);
        wb_tail.j[wb_tail.n++] = j;
        const bool fits = wb_tail.n + pw_query.n <= MAX_WJOBS;
        for (int i = 0; fits && i < pw_query.n; ++i) wb_tail.j[wb_tail.n++] = pw_query.j[i];
        hipStream_t qs = c.s, vs = qfused ? sw : (qlong ? sq : main_s);
        c.order(qs, vs);
        c.s = vs;
        LAUNCH("wgrad", launch_wgrad(wb_tail, c.s));
        if (!fits) LAUNCH("wgrad", launch_wgrad(pw_query, c.s));
        c.s = qs;
    }
    if (!lin_hosted)
        LAUNCH("linear_bwd_data", launch_linear_bwd_data3(c.W(p.dqf), reinterpret_cast<const uint16_t*>(c.PK(K.emb_t3)), c.W(p.dE), Rq, EW, K.emb_t3_cols, c.s));
    {
        const int ebc = embed_bwd_chunk(Rq, p.Lc, cf.char_dim), nce = (Rq + ebc - 1) / ebc;
        const int wtot = cf.char_dim * 300;
        const int64_t ow = c.part_alloc((int64_t)nce * wtot), ob = c.part_alloc((int64_t)nce * 100);
        const int ch[4] = {10, 20, 30, 40};
        int wo = 0, bo = 0;
        for (int i = 0; i < 4; ++i) {
            const int wn = ch[i] * cf.char_dim * (i + 1);
            c.reg(P.ccw[i], wn, p.partial + ow + wo, nce, wtot);
            c.reg(P.ccb[i], ch[i], p.partial + ob + bo, nce, 100);
            wo += wn; bo += ch[i];
        }
        float* p_tab = c.slab(P.char_tab, cf.char_size * cf.char_dim, nce);
        float* p_unk = cf.word_table ? nullptr : c.slab(P.unk, cf.word_dim, nce);
        LAUNCH("embed_bwd", launch_embed_bwd(c.W(p.dE), io->word_ids, io->char_ids, c.W(p.E), reinterpret_cast<const int8_t*>(c.W(p.argpos)),
                                c.P(P.char_tab), c.PK(K.ccw_imgb), c.part_ptr(ow), c.part_ptr(ob), p_tab, p_unk, Rq,
                                p.Lc, cf.word_dim, cf.char_dim, cf.char_size, c.drop(SITE_WORD), c.drop(SITE_CHAR), c.s));
    }
    if (cf.word_table && !c.dry)
        LAUNCH("word_table_bwd", launch_word_table_bwd(c.W(p.dE), io->word_ids, io->grads + P.unk, Rq, cf.word_size, cf.word_dim, c.drop(SITE_WORD), c.s));
    // the loss of vsl_io.fused_loss whose seeds the kernels computed themselves: 64 small workgroups behind the QUERY chain's last kernel (the main
    // stream at T <= 128), in the shadow of the join below (at the headline shape that chain ends ~30 us before the video stream's last weight-gradient
    // batch).  On the weight-gradient stream in front of its first batch it took CUs from the chain's 256-workgroup kernels and cost what it saved
    // (r06 notes 10)
    loss_on_side(c);
    c.s = main_s;
    c.order(sq, c.s);                      // join both side streams before the reduction
    c.order(sw, c.s);
    const int nlate = p.nblocks - p.nblocks_early;
    LAUNCH("reduce", launch_reduce(c.ws, io->grads, p.segs_dev, p.blk2seg_dev + 2 * p.nblocks_early, nlate, p.sq_dev + p.nblocks_early, c.s));
    const vsl_fused_step* fs = c.dry ? nullptr : io->fused_step;
    if (!fs) return;
    // the optimizer step inside the call (vsl_io.fused_step): AdamW behind the reduction (clip norm from the reduction's sums of squares when
    // they cover the whole bucket)
    const vsl_adamw& hp = fs->hp;
    const float bc1 = (float)(1.0 - std::pow((double)hp.beta1, (double)hp.step)), bc2s = (float)std::sqrt(1.0 - std::pow((double)hp.beta2, (double)hp.step));
    LAUNCH("adamw", launch_adamw(fs->params, io->grads, fs->exp_avg, fs->exp_avg_sq, c.h->decay_dev, c.h->opt_scratch, c.h->param_floats, hp.lr,
                                 hp.beta1, hp.beta2, hp.eps, hp.weight_decay, hp.clip_norm, bc1, bc2s, fs->grad_norm_out, c.s, hp.hf_order,
                                 p.sq_cover ? p.sq_dev : nullptr, p.nblocks));
}

}  // namespace vsl
