// The backward launch sequence: run_backward is the stream plan plus a list of stages (loss seeds, span heads, predictor head, fusion, the video
// chain and the query chain behind the fork, the two gradient reductions and the fused AdamW); under the stages one encoder application (enc_bwd),
// the sample-local query pass (query_bwd) and the weight-gradient job helpers both end in.
// THE CONTRACT of this file: a dry run of run_backward (Ctx::dry, build_train_plan) lays out the partial arena of a training plan, so the sequence
// of slab / reg / part_alloc calls IS the arena layout and the order in which k_reduce adds its sources -- it depends on the plan and the handle's
// configuration alone, never on the call.  The sequence of launches, the stream of each and every ordering point are the step's schedule.  Moving
// code between stages must keep all three sequences as they are (tools/host_equivalence.py records them).
#include "host.hpp"

namespace vsl {

namespace {

// what run_backward holds back for a later point of the step and hands to the helpers that add to it or launch it
struct Pending {
    std::vector<WgradBatch> wgrad;      // weight-gradient batches waiting for ONE ordering point (wgrad_async / wgrad_flush)
    bool defer = false;                 // wgrad_async collects instead of launching
    const vsl_loss_io* loss = nullptr;  // vsl_io.fused_loss, not launched yet (loss_on_side)
};

// the loss launch of vsl_io.fused_loss on the current stream (loss_seeds / run_backward decide where: in front of the heads' backward when they read the
// seeds from memory, at the end of the query chain when they compute them)
void loss_on_side(Ctx& c, Pending& pd) {
    const vsl_loss_io* fl = pd.loss;
    if (!fl) return;
    pd.loss = nullptr;
    LAUNCH("loss", launch_loss(LossArgs{c.start_logits(), c.end_logits(), c.h_score(), fl->start_labels, fl->end_labels, fl->h_labels, c.v_mask(), c.p->B, c.p->T,
                                        fl->inv_batch, fl->mask_sum, fl->w_loc, fl->w_highlight, c.W(c.p->loss_scratch), fl->losses, fl->d_start_logits,
                                        fl->d_end_logits, fl->d_h_score, c.h->loss_counter}, c.s));
}
// Every cross-stream ordering point (event record on the producer + wait on the consumer) leaves a ~6-7 us bubble in the
// producer stream (rocprofv3 timeline), so weight-gradient batches -- nothing waits for them before the final reduction --
// are collected while `defer` is set and go to the side stream behind ONE event.
void wgrad_now(Ctx& c, hipStream_t sw, const WgradBatch* wb, size_t n) {       // n > 0 batches on sw, behind everything enqueued so far on c.s
    hipStream_t keep = c.s;
    c.order(keep, sw);
    c.s = sw;
    for (size_t i = 0; i < n; ++i) LAUNCH("wgrad", launch_wgrad(wb[i], c.s));
    c.s = keep;
}
void wgrad_async(Ctx& c, Pending& pd, hipStream_t sw, const WgradBatch& wb) { if (pd.defer) pd.wgrad.push_back(wb); else wgrad_now(c, sw, &wb, 1); }
void wgrad_flush(Ctx& c, Pending& pd, hipStream_t sw) {
    if (!pd.wgrad.empty()) wgrad_now(c, sw, pd.wgrad.data(), pd.wgrad.size());
    pd.wgrad.clear();
}

WgradJob wjob() { WgradJob j; memset(&j, 0, sizeof j); return j; }
WgradBatch wbatch() { WgradBatch wb; memset(&wb, 0, sizeof wb); return wb; }

// The out_layer job and the fused q / k / v job of one encoder application, appended to `wb`; their partial slabs are allocated here, in this order
void attn_wgrad_jobs(Ctx& c, const EncP& P, const EncWs& w, const EncTmp& t, WgradBatch& wb) {
    const Plan& p = *c.p;
    const int R = w.R, nchunk = (R + WG_ROWS - 1) / WG_ROWS;
    {
        WgradJob j = wjob();
        j.G[0] = c.W(t.go); j.nG = 1; j.A[0] = c.W(w.h2); j.nA = 1; j.K = D; j.R = R;
        j.out = c.slab(P.ow, D * D, nchunk);
        j.out_bias[0] = c.slab(P.ob, D, nchunk);
        wb.j[wb.n++] = j;
    }
    {
        WgradJob j = wjob();
        j.G[0] = c.W(t.dq); j.G[1] = c.W(t.dk); j.G[2] = c.W(t.dv); j.A[0] = c.W(w.h1);
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

// the four pointwise-conv jobs of one encoder application, appended to `wb`, in chunks of `rows` rows (0 = WG_ROWS)
void pointwise_wgrad_jobs(Ctx& c, const EncP& P, const EncWs& w, const EncTmp& t, WgradBatch& wb, int rows) {
    for (int i = 0; i < 4; ++i) {
        WgradJob j = wjob();
        j.G[0] = c.W(t.gz[i]); j.A[0] = c.W(w.u[i]);
        j.nG = 1; j.nA = 1; j.K = D; j.R = w.R;
        j.rows = rows;
        const int nch_pw = wgrad_chunks(w.R, wgrad_rows(j));
        j.out = c.slab(P.pw[i], D * D, nch_pw);
        j.out_bias[0] = c.slab(P.pwb[i], D, nch_pw);
        wb.j[wb.n++] = j;
    }
}

// the attention-output backward of encoder application `app` (its LayerNorm-2 partial slabs are allocated here: call once per application)
AttnOutBwdArgs attn_out_bwd_args(Ctx& c, const EncP& P, const EncPk& K, const EncWs& w, const float* dy, const float* dy2, int app) {
    const EncTmp& t = c.p->tmp[app];
    const int ntiles = (w.R + TILE_M - 1) / TILE_M;
    float* p_ln2g = c.slab(P.ln2g, D, ntiles);
    float* p_ln2b = c.slab(P.ln2b, D, ntiles);
    return AttnOutBwdArgs{dy, dy2, c.W(w.r), c.P(P.ln2g), c.PK(K.o_t), c.W(t.go), c.W(t.dr), p_ln2g, p_ln2b, c.drop(app * 16 + 7), c.drop(app * 16 + 8)};
}

// What the conv block's backward workgroups go on with on their tile of dx0 (CbBwdArgs::tail): nothing, the attention-output backward of the pass
// below, the CQConcatenate backward, or the Embedding linear's data gradient.  The caller has checked that the kernel hosts it
// (convblock_bwd_hosts_tail / convblock_bwd_hosts_linear) and skips that launch.
struct LinTail { const uint16_t* WT3; float* dA; int K, Kc; };
struct ConvTail {
    int kind = 0;                       // CbBwdArgs::tail: 0 nothing, 1 `ao`, 2 `cq`, 3 `lin` -- the one member that counts
    AttnOutBwdArgs ao; CqcatBwdArgs cq; LinTail lin;
    static ConvTail attn_out(const AttnOutBwdArgs& a) { ConvTail t{}; t.kind = 1; t.ao = a; return t; }
    static ConvTail cqcat(const CqcatBwdArgs& a) { ConvTail t{}; t.kind = 2; t.cq = a; return t; }
    static ConvTail linear(const LinTail& a) { ConvTail t{}; t.kind = 3; t.lin = a; return t; }
};
struct EncBwdOpts {
    bool attn_out_done = false;         // the attention-output backward of this application already ran (inside the span heads' kernel or a conv block's tail)
    ConvTail tail{};
    int pw_rows = 0;                    // rows per chunk of the pointwise weight-gradient jobs (0 = WG_ROWS)
    WgradBatch* pw_out = nullptr;       // hand the pointwise batch back instead of launching it on `sw`: the caller launches it on a stream of its
                                        // own choice WITHOUT a cross-stream wait (each costs ~16 us)
};
// Backward of one FeatureEncoder application.  dy (+ dy2) = grad wrt its output; writes grad wrt its input to the workspace at dx0_off (whose per-sample
// rows are also the positional table's partial slabs); `mask` (Bn, L); sw: stream of the out_layer / q,k,v weight gradients and, unless handed back, the
// pointwise ones.  Enqueues on c.s: [attn_out_bwd] attn_bwd [qkv_bwd] convblock_bwd.
void enc_bwd(Ctx& c, Pending& pd, const EncP& P, const EncPk& K, const EncWs& w, const float* dy, const float* dy2, int64_t dx0_off, const float* mask,
             int Bn, int app, hipStream_t sw, const EncBwdOpts& o = EncBwdOpts{}) {
    const EncTmp& t = c.p->tmp[app];
    const int R = w.R, L = w.L, H = c.h->cfg.num_heads;
    const int ntiles = (R + TILE_M - 1) / TILE_M;
    if (!o.attn_out_done) {
        const AttnOutBwdArgs ao = attn_out_bwd_args(c, P, K, w, dy, dy2, app);
        LAUNCH("attn_out_bwd", launch_attn_out_bwd(ao, R, c.s));
    }
    // every head count, every L: key-major dK / dV; dQ as attn_dq_slabs(L) slabs (L > ATTN_SLAB_MAX_L: query-major into slab 0, kernels_attn.hip)
    LAUNCH("attn_bwd", launch_attn_bwd(AttnArgs{c.W(w.q), c.W(w.k), c.W(w.v), mask, c.W(w.att), c.W(w.lse), c.W(t.dr), c.W(t.dq), c.W(t.dk), c.W(t.dv),
                                                Bn, L, H, 0, c.drop(app * 16 + 5), c.drop(app * 16 + 6)}, c.s));
    // whole tiles / sample tiles (and one dQ slab): the conv block's backward kernel computes its own incoming gradient from dq / dk / dv (CbBwdArgs::qk).
    // The gate stays on the key-major slab count: L > 256 never fuses, the one-slab dQ of L > ATTN_SLAB_MAX_L included (k_qkv_bwd adds nothing there)
    static const bool fuse_on = switch_on("VSL_QKV_FUSED", true);
    const bool fuse_qkv = fuse_on && convblock_bwd_hosts_qkv(R, L) && attn_bwd_dq_slabs(L) == 1;
    const int nsl1 = fuse_qkv ? convblock_slabs(R, L) : ntiles;
    float* p_ln1g = c.slab(P.ln1g, D, nsl1);
    float* p_ln1b = c.slab(P.ln1b, D, nsl1);
    const uint16_t* WqkvT3 = reinterpret_cast<const uint16_t*>(c.PK(K.qkv_t3));
    if (!fuse_qkv)
        LAUNCH("qkv_bwd", launch_qkv_bwd(c.W(t.dq), c.W(t.dk), c.W(t.dv), c.W(w.y[3]), c.W(t.dr), c.P(P.ln1g), WqkvT3, c.W(t.ga), p_ln1g, p_ln1b, R,
                                         c.drop(app * 16 + 4), c.s, attn_dq_slabs(L)));
    {   // out_layer + fused q/k/v weight gradients: every input exists now -> side stream, beside the conv chain
        WgradBatch wb = wbatch();
        attn_wgrad_jobs(c, P, w, t, wb);
        wgrad_async(c, pd, sw, wb);
    }
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
        const ConvTail& tl = o.tail;
        a.tail = tl.kind; a.tail_ao = tl.ao; a.tail_cq = tl.cq; a.tail_lin_WT3 = tl.lin.WT3; a.tail_lin_dA = tl.lin.dA; a.tail_lin_K = tl.lin.K; a.tail_lin_Kc = tl.lin.Kc;
        if (fuse_qkv) {
            a.qkv = 1;
            a.qk = QkvBwdFuse{c.W(t.dq), c.W(t.dk), c.W(t.dv), c.W(w.y[3]), c.W(t.dr), c.P(P.ln1g), WqkvT3, p_ln1g, p_ln1b, c.drop(app * 16 + 4)};
        }
        a.dy = c.W(t.ga); a.dx0 = c.W(dx0_off); a.R = R; a.L = L;
        for (int i = 0; i < 4; ++i) {
            a.x[i] = i > 0 ? c.W(w.y[i - 1]) : c.W(w.x0);
            a.relu_mask[i] = reinterpret_cast<const uint32_t*>(c.W(w.mask[i]));
            a.ln_g[i] = c.P(P.lng[i]); a.ln_b[i] = c.P(P.lnb[i]); a.dw_w[i] = c.P(P.dw[i]);
            a.dp[i] = c.drop(app * 16 + i); a.gz[i] = c.W(t.gz[i]);
            a.WT3[i] = reinterpret_cast<const uint16_t*>(c.PK(K.pw_t3[i]));
        }
        LAUNCH("convblock_bwd", launch_convblock_bwd(a, c.s));
    }
    {   // pointwise-conv weight gradients (inputs complete only now); Wo / QKV were launched right after qkv_bwd
        WgradBatch wb = wbatch();
        pointwise_wgrad_jobs(c, P, w, t, wb, o.pw_rows);
        if (o.pw_out) *o.pw_out = wb;
        else wgrad_async(c, pd, sw, wb);
    }
    // positional table (:202): dpos[t] = sum_b dx0[b, t] -- the per-sample rows of dx0 ARE the partial slabs
    c.reg(P.pos, c.h->cfg.max_pos_len * D, dx0_off, Bn, L * D, 0, 0, L * D);
}

// the query pass' backward as ONE sample-local launch (kernels_query.hip: k_query_bwd) + the weight-gradient jobs that read what it leaves, appended
// to `jobs`: out_layer, fused q/k/v, the four pointwise convs (the Embedding linear's job is the caller's: it also owns dqf / E)
void query_bwd(Ctx& c, const float* dy, int64_t dx0_off, WgradBatch& jobs) {
    const vsl_config& cf = c.h->cfg; const ModelPk& MK = c.h->K; const EncP& P = c.h->P.fe; const EncPk& K = c.h->K.fe;
    const Plan& p = *c.p; const EncWs& w = p.qe; const EncTmp& t = p.tmp[1];
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
    a.dout = dy; a.r = c.W(w.r); a.ln2_g = c.P(P.ln2g); a.WoT3 = reinterpret_cast<const uint16_t*>(c.PK(K.o_t3)); a.go = c.W(t.go);
    a.d2 = c.drop(app * 16 + 5); a.d3 = c.drop(app * 16 + 6); a.d4 = c.drop(app * 16 + 7); a.d5 = c.drop(app * 16 + 8);
    a.q = c.W(w.q); a.k = c.W(w.k); a.v = c.W(w.v); a.att = c.W(w.att); a.lse = c.W(w.lse); a.mask = c.q_mask();
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
    LAUNCH("query_bwd", launch_query_bwd(a, B, c.s));
    attn_wgrad_jobs(c, P, w, t, jobs);
    pointwise_wgrad_jobs(c, P, w, t, jobs, 0);
    c.reg(P.pos, cf.max_pos_len * D, dx0_off, B, Lq * D, 0, 0, Lq * D);     // positional table (:202): the per-sample rows of dx0 are the partial slabs
}

// ---- the stages of run_backward: each enqueues on c.s (and on the streams it is given) and reads nothing but its arguments, the plan and the
// call's vsl_io

// Where the consumers of the loss seeds -- the span heads' backward, the highlight layer's -- find them.
// vsl_io.fused_loss: the loss is part of this call.  Whole tiles + the caller's mask sum (`inline_fl`): k_loss_fused leaves the dependent chain
// (nothing on it reads what the kernel writes; run_backward launches it at the end of the query chain) and the consumers compute the seeds from the
// logits themselves.  Otherwise the loss launches first, here, on the caller's stream, and the seeds are read from memory as they always were.
struct HlSeed { const int64_t* h_lab; const float* vmask; float w_hl, mask_sum; };     // (the inline highlight seed of CqcatBwdArgs: cqcat_bwd_args copies it in)
struct LossSeeds {
    const float *s, *e, *h;             // dLoss / d start_logits, end_logits, h_score in memory
    const vsl_loss_io* inline_fl;       // non-null: computed in the consumers from the logits and these labels / weights
    HlSeed hl;                          // the highlight layer's share of that (h_lab == nullptr: read `h`)
};
LossSeeds loss_seeds(Ctx& c, Pending& pd) {
    LossSeeds sd{c.d_start_logits(), c.d_end_logits(), c.d_h_score(), nullptr, HlSeed{nullptr, nullptr, 0.f, 0.f}};
    const vsl_loss_io* fl = c.fused_loss();
    if (!fl) return sd;
    static const bool inline_on = switch_on("VSL_LOSS_INLINE", true);
    const bool seeds_inline = inline_on && c.p->T >= TILE_M && fl->mask_sum > 0.f && c.h->loss_counter != nullptr;       // (T >= 32: a row tile touches at most two samples)
    pd.loss = fl;
    if (!seeds_inline) loss_on_side(c, pd);            // (here and now, on the caller's stream: the seeds are read from memory)
    else { sd.inline_fl = fl; sd.hl = HlSeed{fl->h_labels, c.v_mask(), fl->w_highlight, fl->mask_sum}; }
    return sd;
}

// the span heads and their weight-gradient batch ; transformer head: the end head's workgroups run the attention-output backward of the second
// predictor pass on their own tile of dfeat_e
void heads_bwd(Ctx& c, Pending& pd, const LossSeeds& sd, hipStream_t sw) {
    const ModelP& P = c.h->P; const ModelPk& K = c.h->K; const Plan& p = *c.p;
    const bool rnn = c.h->cfg.predictor == 0;
    const int R = p.B * p.T, ntiles = (R + TILE_M - 1) / TILE_M, nchunk = (R + WG_ROWS - 1) / WG_ROWS;
    HeadBwdArgs hs{sd.s, c.W(p.hid_s), c.W(p.p1.out), rnn ? nullptr : c.P(P.sln_g), c.PK(K.s0_t), c.P(P.s1w), c.W(p.gz_s),
                   c.W(p.dfeat_s), c.W(p.dxh_s), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0};
    HeadBwdArgs he{sd.e, c.W(p.hid_e), c.W(p.p2.out), rnn ? nullptr : c.P(P.eln_g), c.PK(K.e0_t), c.P(P.e1w), c.W(p.gz_e),
                   c.W(p.dfeat_e), c.W(p.dxh_e), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0};
    if (const vsl_loss_io* fl = sd.inline_fl) {
        hs.logits = c.start_logits(); hs.label = fl->start_labels; hs.cs = fl->w_loc * fl->inv_batch; hs.T = p.T;
        he.logits = c.end_logits(); he.label = fl->end_labels; he.cs = fl->w_loc * fl->inv_batch; he.T = p.T;
    }
    hs.p_b0 = c.slab(P.s0b, D, ntiles); hs.p_w1 = c.slab(P.s1w, D, ntiles); hs.p_b1 = c.slab(P.s1b, 1, ntiles);
    he.p_b0 = c.slab(P.e0b, D, ntiles); he.p_w1 = c.slab(P.e1w, D, ntiles); he.p_b1 = c.slab(P.e1b, 1, ntiles);
    if (!rnn) {
        hs.p_lng = c.slab(P.sln_g, D, ntiles); hs.p_lnb = c.slab(P.sln_b, D, ntiles);
        he.p_lng = c.slab(P.eln_g, D, ntiles); he.p_lnb = c.slab(P.eln_b, D, ntiles);
    }
    AttnOutBwdArgs ao2;
    if (!rnn) ao2 = attn_out_bwd_args(c, P.pe, K.pe, p.p2, nullptr, nullptr, 3);
    LAUNCH("head_bwd", launch_head_bwd(hs, he, R, c.s, rnn ? nullptr : &ao2));
    WgradBatch wb = wbatch();
    for (int e = 0; e < 2; ++e) {
        WgradJob j = wjob();
        j.G[0] = c.W(e ? p.gz_e : p.gz_s); j.A[0] = rnn ? c.W(p.lstm[e].out) : c.W(e ? p.lnf_e : p.lnf_s); j.A[1] = c.W(p.gated);
        j.nG = 1; j.nA = 2; j.K = 2 * D; j.R = R;
        j.out = c.slab(e ? P.e0w : P.s0w, D * 2 * D, nchunk);
        wb.j[wb.n++] = j;
    }
    wgrad_async(c, pd, sw, wb);
}

// rnn head: BPTT through the end LSTM, then the start LSTM (whose output also feeds the start span block), into g_gated; then the weight gradients.
// Pipelined in time chunks like the forward (fuse_and_predict): the end LSTM walks the chunks backwards on the main stream; behind it the side
// stream turns the chunk's gate gradients into the start LSTM's incoming gradient (dx = dG W_ih, row-mapped GEMM) and runs the start LSTM over the
// same chunk.
void rnn_head_bwd(Ctx& c, hipStream_t sw, hipStream_t sq) {
    const ModelP& P = c.h->P; const ModelPk& K = c.h->K; const Plan& p = *c.p;
    const int B = p.B, T = p.T, R = B * T, nchunk = (R + WG_ROWS - 1) / WG_ROWS;
    const std::vector<int> chunks = lstm_chunks(T);
    auto bwd = [&](int l, int t0, int t1) {
        const LstmWs& w = p.lstm[l];
        LAUNCH("lstm_bwd", launch_lstm_bwd(c.W(l ? p.dfeat_e : p.dfeat_s), l ? nullptr : c.W(p.g_s1), c.v_mask(), c.W(w.gates), c.W(w.cseq), c.W(w.tseq),
                                           c.P(P.l_whh[l]), c.PK(K.l_hb[l]), c.W(w.dG), B, T, c.s, c.W(w.carry), t0, t1));
    };
    // dx = dG W_ih : (rows,512) x (512,128), K-streamed GEMM kernel of the visual projection, no dropout, zero bias
    auto dx = [&](int l, int t0, int t1) {
        const LstmWs& w = p.lstm[l];
        const bool all = t0 == 0 && t1 == T;
        LAUNCH("lstm_dx", launch_vproj_fwd3(c.W(w.dG), reinterpret_cast<const uint16_t*>(c.PK(K.l_t3[l])), c.PK(K.zero128), c.W(l ? p.g_s1 : p.g_gated),
                                           all ? R : B * (t1 - t0), 4 * D, Drop{0u, 0u, 1.f}, c.s, all ? 0 : t1 - t0, T, t0));
    };
    if (p.h_gran >= 0) {
        RnnBwdArgs a;
        memset(&a, 0, sizeof a);
        a.dout[0] = c.W(p.dfeat_s); a.dout[1] = c.W(p.dfeat_e); a.mask = c.v_mask(); a.Wih1 = c.PK(K.l_ib);
        for (int l = 0; l < 2; ++l) {
            const LstmWs& w = p.lstm[l];
            a.gates[l] = c.W(w.gates); a.cseq[l] = c.W(w.cseq); a.tseq[l] = c.W(w.tseq); a.Whh[l] = c.PK(K.l_hb[l]); a.dG[l] = c.W(w.dG);
        }
        a.dg_gran = reinterpret_cast<unsigned long long*>(c.W(p.dg_gran)); a.dx_gran = reinterpret_cast<unsigned long long*>(c.W(p.dx_gran));
        a.B = B; a.T = T;
        if (!c.dry) {                       // (the launch's tag and the memset it may need: process-wide counters a plan build must not move)
            long long gen = 0;
            a.epoch = rnn_epoch(&gen);
            rnn_granules_fresh(c, *c.p, gen);
        }
        LAUNCH("rnn_bwd", launch_rnn_bwd(a, c.s));
        dx(0, 0, T);
    } else if (chunks.size() < 2 || sq == c.s) {
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
    for (int l = 1; l >= 0; --l) {
        const LstmWs& w = p.lstm[l];
        // weight gradients: dW_ih = dG^T x, dW_hh = dG^T h_prev, db_ih = db_hh = column sums of dG (two gate pairs per job)
        WgradBatch wb = wbatch();
        for (int which = 0; which < 2; ++which) {                     // 0: W_ih (+ biases), 1: W_hh
            for (int half = 0; half < 2; ++half) {
                WgradJob j = wjob();
                j.G[0] = c.W(w.dG + (2 * half) * D); j.G[1] = c.W(w.dG + (2 * half + 1) * D);
                j.A[0] = which ? c.W(w.hprev) : (l ? c.W(p.lstm[0].out) : c.W(p.gated));
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
        wgrad_now(c, sw, &wb, 1);
    }
}

// the highlight layer's partial slabs and the arguments of the gating + HighLightLayer + CQConcatenate backward (dg0 = grad wrt the gated features
// through the predictor; nullptr when a conv block's tail supplies its own dx0)
CqcatBwdArgs cqcat_bwd_args(Ctx& c, const LossSeeds& sd, const float* dg0) {
    const ModelP& P = c.h->P; const Plan& p = *c.p;
    const int ntiles = (p.B * p.T + TILE_M - 1) / TILE_M;
    float* p_hlw = c.slab(P.hl_w, D, ntiles);
    float* p_hlb = c.slab(P.hl_b, 1, ntiles);
    return CqcatBwdArgs{dg0, c.W(p.dxh_s), c.W(p.dxh_e), sd.h, c.W(p.f2), c.h_score(), c.P(P.hl_w), c.PK(c.h->K.cat1_t), c.W(p.df2), c.W(p.df1), p_hlw, p_hlb,
                        sd.hl.h_lab, sd.hl.vmask, sd.hl.w_hl, sd.hl.mask_sum};
}

// transformer head: the predictor encoder's second pass (input = output of the first pass), then the first, into g_gated.  Whole tiles (returns true):
// tile-local continuations inside the conv block's backward kernel -- pass 2's conv block goes on with pass 1's attention-output backward (dy = its
// dx0 + the start head's LayerNorm path), pass 1's with the CQConcatenate backward (dg0 = its dx0), which fusion_bwd then does not launch.
bool transformer_head_bwd(Ctx& c, Pending& pd, const LossSeeds& sd, hipStream_t sw) {
    const ModelP& P = c.h->P; const ModelPk& K = c.h->K; const Plan& p = *c.p;
    const bool hosted = convblock_bwd_hosts_tail(p.B * p.T, p.T);
    EncBwdOpts o2, o1;
    o2.attn_out_done = true;                // (inside the span heads' kernel: heads_bwd)
    if (hosted) o2.tail = ConvTail::attn_out(attn_out_bwd_args(c, P.pe, K.pe, p.p1, nullptr, c.W(p.dfeat_s), 2));
    enc_bwd(c, pd, P.pe, K.pe, p.p2, c.W(p.dfeat_e), nullptr, p.g_s1, c.v_mask(), p.B, 3, sw, o2);
    wgrad_flush(c, pd, sw);   // span heads + pass-2 weight gradients: one ordering point
    // grad wrt the first pass' output = (input grad of the second pass) + (LayerNorm path of the start head)
    o1.attn_out_done = hosted;
    if (hosted) o1.tail = ConvTail::cqcat(cqcat_bwd_args(c, sd, nullptr));
    enc_bwd(c, pd, P.pe, K.pe, p.p1, c.W(p.g_s1), c.W(p.dfeat_s), p.g_gated, c.v_mask(), p.B, 2, sw, o1);
    return hosted;
}

// gating + highlight + CQConcatenate (unless a conv block hosted it: `cqcat_done`), their weight gradients -- the last batch behind the deferred
// ordering point -- and CQAttention + WeightedPool / pooled-bias backward as four tile-parallel kernels (kernels_cq_bwd.hip), three of them here: dC is
// final; the fourth (launch_cq_bwd_query, same arguments: the returned struct) opens the query chain
CqBwdArgs fusion_bwd(Ctx& c, Pending& pd, const LossSeeds& sd, bool cqcat_done, hipStream_t sw) {
    const ModelP& P = c.h->P; const ModelPk& K = c.h->K; const Plan& p = *c.p;
    const int B = p.B, T = p.T, R = B * T, nchunk = (R + WG_ROWS - 1) / WG_ROWS;
    if (!cqcat_done) {
        const CqcatBwdArgs a = cqcat_bwd_args(c, sd, c.W(p.g_gated));
        LAUNCH("cqcat_bwd", launch_cqcat_bwd(a, R, c.s));
    }
    WgradBatch wb = wbatch();
    {   // first half of the (128, 256) CQConcatenate weight: destination rows are strided by 256
        WgradJob j = wjob();
        j.G[0] = c.W(p.df2); j.A[0] = c.W(p.f1);
        j.nG = 1; j.nA = 1; j.K = D; j.R = R;
        const int64_t o = c.part_alloc((int64_t)nchunk * D * D);
        c.reg(P.cat_w, D * D, p.partial + o, nchunk, D * D, D, 2 * D);
        j.out = c.part_ptr(o);
        wb.j[wb.n++] = j;
    }
    {   // cqa_linear (128, 512)
        WgradJob j = wjob();
        j.G[0] = c.W(p.df1); j.Afull = c.W(p.cat);
        j.nG = 1; j.nA = 0; j.K = 4 * D; j.R = R;
        j.out = c.slab(P.cqa_w, D * 4 * D, nchunk);
        j.out_bias[0] = c.slab(P.cqa_b, D, nchunk);
        wb.j[wb.n++] = j;
    }
    wgrad_async(c, pd, sw, wb);
    wgrad_flush(c, pd, sw);                 // pass-1 + fusion weight gradients: one ordering point
    pd.defer = false;
    const int ntile = (T + TILE_M - 1) / TILE_M;
    CqBwdArgs q;
    memset(&q, 0, sizeof q);
    q.df1 = c.W(p.df1); q.df2 = c.W(p.df2); q.C = c.W(p.ve.out); q.Qf = c.W(p.qe.out); q.Srow = c.W(p.Srow);
    q.Scol = c.W(p.Scol); q.M = c.W(p.M); q.alpha = c.W(p.alpha); q.pooled = c.W(p.pooled); q.WcqaT = c.PK(K.cqa_t);
    q.w4C = c.P(P.w4C); q.w4Q = c.P(P.w4Q); q.w4mlu = c.P(P.w4mlu); q.pool_w = c.P(P.pool_w); q.Wcat = c.P(P.cat_w);
    q.dC = c.W(p.dC); q.dQ = c.W(p.dQtot); q.dSr = c.W(p.dSr); q.dSs = c.W(p.dSs);
    q.P1 = c.W(p.cqP1); q.P2 = c.W(p.cqP2); q.P3 = c.W(p.cqP3); q.P4 = c.W(p.cqP4); q.P5 = c.W(p.cqP5);
    q.vidx = c.video_index();               // shared step: C is the (Nv, T, 128) encoding; dC stays (B, T, 128)
    q.T = T; q.Lq = p.Lq; q.b_off = 0; q.dc = c.drop(SITE_CQ_C); q.dq = c.drop(SITE_CQ_Q);
    q.p_w4C = c.slab(P.w4C, D, B * ntile); q.p_w4mlu = c.slab(P.w4mlu, D, B * ntile);
    q.p_w4Q = c.slab(P.w4Q, D, B); q.p_pool = c.slab(P.pool_w, D, B); q.p_bcat = c.slab(P.cat_b, D, B);
    const int64_t o = c.part_alloc((int64_t)B * D * D);
    c.reg(P.cat_w + D, D * D, p.partial + o, B, D * D, D, 2 * D);          // second half of the (128, 256) weight
    q.p_W2 = c.part_ptr(o);
    LAUNCH("cq_bwd", launch_cq_bwd(q, B, c.s));
    return q;
}

// The video chain on c.s: the shared step's group_sum, encoder application 0 over the plan's video half (Nv T rows), then VisualProjection's weight
// gradient back to back, no waits.  Sample-local query path: the video pass' pointwise weight gradients ride in that launch (nothing on the video
// stream waits for the query chain any more); otherwise they are handed back in `pw_video` for the query chain's tail batch.
// (Measured and dropped: the video pass' pointwise batch on the weight-gradient stream instead, +3.5 %: profiles/r06_notes.md)
void video_chain_bwd(Ctx& c, Pending& pd, hipStream_t sw, WgradBatch& pw_video) {
    const vsl_config& cf = c.h->cfg; const ModelP& P = c.h->P; const Plan& p = *c.p;
    const bool shared = p.kind == PlanKind::TrainShared;
    const int Nv = p.NV(), Rv = Nv * p.T;
    // The step's LAST weight-gradient batch (VisualProjection + the video pass' four pointwise gradients, sample-local query path) starts into an
    // empty chip: chunk rows that make it whole rounds of one-workgroup-per-CU chunks (Dv = 1024: 12 blocks x 32 chunks = 1.5 rounds -> 400 rows,
    // 252 workgroups; profiles/r06_notes.md section 8: -0.6 % against 256-row chunks).
    const int tail_rows = query_fused(c) ? wgrad_rows_whole_rounds(Rv, (cf.video_feature_dim + 127) / 128 + 4, c.h->cus) : WG_ROWS;
    EncBwdOpts o;
    o.pw_rows = tail_rows == WG_ROWS ? 0 : tail_rows;
    o.pw_out = &pw_video;
    // shared encoding: dCv[n] = the sum of dC[b] over the queries of video n in ascending b (kernels_shared.hip; the CSR is the forward's), a
    // stand-alone launch at the head of the video chain
    if (shared)
        LAUNCH("group_sum", launch_group_sum(c.W(p.dC), reinterpret_cast<const int*>(c.W(p.csr)), reinterpret_cast<const int*>(c.W(p.csr + p.csr_members())),
                                             c.W(p.dCv), Nv, p.T, c.s));
    enc_bwd(c, pd, P.fe, c.h->K.fe, p.ve, c.W(shared ? p.dCv : p.dC), nullptr, p.dvf, c.video_mask(), Nv, 0, sw, o);
    WgradBatch wb = wbatch();
    WgradJob j = wjob();
    j.rows = o.pw_rows;
    const int nchunk = wgrad_chunks(Rv, tail_rows);
    j.G[0] = c.W(p.dvf); j.Afull = c.video_features();
    if (c.video_features_bf16()) { j.Afull = reinterpret_cast<const float*>(c.video_features_bf16()); j.a_bf16 = 1; }
    j.nG = 1; j.nA = 0; j.K = cf.video_feature_dim; j.R = Rv; j.drop_on_A = 1; j.dp = c.drop(SITE_VIS);
    j.out = c.slab(P.va_w, D * cf.video_feature_dim, nchunk);
    j.out_bias[0] = c.slab(P.va_b, D, nchunk);
    wb.j[wb.n++] = j;
    if (query_fused(c)) { for (int i = 0; i < pw_video.n; ++i) wb.j[wb.n++] = pw_video.j[i]; }
    LAUNCH("wgrad", launch_wgrad(wb, c.s));
}

// The query chain on c.s: the fourth CQ kernel (dQ: only the query side consumes it), the query pass, the embedding stack and the deferred loss.
// Every remaining weight gradient (the query pass', the Embedding linear's and -- row-tile query path -- the video pass' pointwise ones) goes as ONE
// batch to `vs`: the weight-gradient stream on the sample-local path, the video chain's stream otherwise, beside the embedding backward that ends
// this chain.
void query_chain_bwd(Ctx& c, Pending& pd, const CqBwdArgs& q, const WgradBatch& pw_video, hipStream_t sw, hipStream_t video_s) {
    const vsl_config& cf = c.h->cfg; const ModelP& P = c.h->P; const ModelPk& K = c.h->K; const Plan& p = *c.p;
    const int B = p.B, Lq = p.Lq, Rq = B * Lq, nchunk_q = (Rq + WG_ROWS - 1) / WG_ROWS, EW = cf.word_dim + 100;
    LAUNCH("cq_bwd_d", launch_cq_bwd_query(q, B, c.s));
    WgradBatch pw_query = wbatch();
    // sample tiles (Lq <= 32): the query pass' conv-block backward goes on with the Embedding linear's data gradient on its rows of dx0
    const bool qfused = query_fused(c);
    const bool lin_hosted = qfused || (convblock_bwd_hosts_linear(Rq, Lq) && K.emb_t3_cols % 512 == 0);
    if (qfused) query_bwd(c, c.W(p.dQtot), p.dqf, pw_query);
    else {
        EncBwdOpts o;
        o.pw_out = &pw_query;
        if (lin_hosted) o.tail = ConvTail::linear(LinTail{reinterpret_cast<const uint16_t*>(c.PK(K.emb_t3)), c.W(p.dE), EW, K.emb_t3_cols});
        enc_bwd(c, pd, P.fe, K.fe, p.qe, c.W(p.dQtot), nullptr, p.dqf, c.q_mask(), B, 1, sw, o);
    }
    {
        WgradBatch wb_tail = pw_video;
        if (qfused) wb_tail.n = 0;
        WgradJob j = wjob();
        j.G[0] = c.W(p.dqf); j.Afull = c.W(p.E);
        j.nG = 1; j.nA = 0; j.K = EW; j.R = Rq;
        j.out = c.slab(P.emb_w, D * EW, nchunk_q);
        j.out_bias[0] = c.slab(P.emb_b, D, nchunk_q);
        wb_tail.j[wb_tail.n++] = j;
        const bool fits = wb_tail.n + pw_query.n <= MAX_WJOBS;
        for (int i = 0; fits && i < pw_query.n; ++i) wb_tail.j[wb_tail.n++] = pw_query.j[i];
        hipStream_t qs = c.s, vs = qfused ? sw : video_s;
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
        LAUNCH("embed_bwd", launch_embed_bwd(EmbedBwdArgs{c.W(p.dE), c.word_ids(), c.char_ids(), c.W(p.E), reinterpret_cast<const int8_t*>(c.W(p.argpos)),
                                                          c.P(P.char_tab), c.PK(K.ccw_imgb), c.part_ptr(ow), c.part_ptr(ob), p_tab, p_unk, Rq, p.Lc, cf.word_dim,
                                                          cf.char_dim, cf.char_size, c.drop(SITE_WORD), c.drop(SITE_CHAR)}, c.s));
    }
    if (cf.word_table)
        LAUNCH("word_table_bwd", launch_word_table_bwd(c.W(p.dE), c.word_ids(), c.grads() + P.unk, Rq, cf.word_size, cf.word_dim, c.drop(SITE_WORD), c.accumulate, c.s));
    // the loss of vsl_io.fused_loss whose seeds the kernels computed themselves: 64 small workgroups behind the QUERY chain's last kernel (the main
    // stream at T <= 128), in the shadow of the join (at the headline shape that chain ends ~30 us before the video stream's last weight-gradient
    // batch).  On the weight-gradient stream in front of its first batch it took CUs from the chain's 256-workgroup kernels and cost what it saved
    // (r06 notes 10)
    loss_on_side(c, pd);
}

}  // namespace

void run_backward(Ctx& c) {
    const vsl_config& cf = c.h->cfg;
    const Plan& p = *c.p;
    // streams: `main` carries the dependent dX chain; sw = every weight-gradient GEMM (they only feed the final
    // reduction); sq = the query-side chain (query encoder pass + embedding stack) once CQAttention's backward is done
    hipStream_t sw = c.s, sq = c.s;         // (a dry run has no streams: everything 'runs' on its null c.s)
    if (!c.dry) { sw = c.side(1); sq = c.side(0); }
    Pending pd;
    pd.defer = !c.dry && cf.predictor == 1;
    const LossSeeds sd = loss_seeds(c, pd);
    heads_bwd(c, pd, sd, sw);
    bool cqcat_done = false;
    if (cf.predictor == 0) rnn_head_bwd(c, sw, sq);
    else cqcat_done = transformer_head_bwd(c, pd, sd, sw);
    const CqBwdArgs q = fusion_bwd(c, pd, sd, cqcat_done, sw);
    // early reduction (predictor / heads / CQ parameters): all their partials exist once the launches above are done
    // (the pooled-query parameters of k_cq_bwd_d belong to the late reduction: that kernel opens the query chain below).
    // ONE event for both consumers: the early reduction on sw and the fork of the query side onto sq
    hipStream_t main_s = c.s;
    c.order2(main_s, sw, sq);
    c.s = sw;
    LAUNCH("reduce", launch_reduce(c.ws, c.grads(), p.segs_dev, p.blk2seg_dev, p.nblocks_early, p.sq_dev, c.accumulate, c.s));
    // data parallel: the predictor block of the gradient bucket is final now -- the caller's all-reduce of it can start (vslnet_hip.h)
    if (!c.dry && c.io->early_grads_event && cf.predictor == 1) (void)hipEventRecord((hipEvent_t)c.io->early_grads_event, sw);
    // from here the video side and the query side are independent; the longer one keeps the main stream
    const bool qlong = query_chain_is_longer(p);
    hipStream_t video_s = qlong ? sq : main_s, query_s = qlong ? main_s : sq;
    WgradBatch pw_video = wbatch();
    c.s = video_s;
    video_chain_bwd(c, pd, sw, pw_video);
    c.s = query_s;
    query_chain_bwd(c, pd, q, pw_video, sw, video_s);
    c.s = main_s;
    c.order(sq, c.s);                      // join both side streams before the reduction
    c.order(sw, c.s);
    LAUNCH("reduce", launch_reduce(c.ws, c.grads(), p.segs_dev, p.blk2seg_dev + 2 * p.nblocks_early, p.nblocks - p.nblocks_early, p.sq_dev + p.nblocks_early, c.accumulate, c.s));
    const vsl_fused_step* fs = c.fused_step();
    if (!fs) return;
    // the optimizer step inside the call (vsl_io.fused_step): AdamW behind the reduction (clip norm from the reduction's sums of squares when
    // they cover the whole bucket)
    const vsl_adamw& hp = fs->hp;
    const float bc1 = (float)(1.0 - std::pow((double)hp.beta1, (double)hp.step)), bc2s = (float)std::sqrt(1.0 - std::pow((double)hp.beta2, (double)hp.step));
    LAUNCH("adamw", launch_adamw(AdamwArgs{fs->params, c.grads(), fs->exp_avg, fs->exp_avg_sq, c.h->decay_dev, c.h->opt_scratch, c.h->param_floats, hp.clip_norm,
                                           AdamHp{hp.lr, hp.beta1, hp.beta2, hp.eps, hp.weight_decay, bc1, bc2s, hp.hf_order}, fs->grad_norm_out,
                                           p.sq_cover ? p.sq_dev : nullptr, p.nblocks}, c.s));
}

// vsl_input_grads: dX = dropmask * (d_video_affine W) over the rows of the plan's video half (N T in a shared step, where dvf already holds each
// video's gradient summed over its queries).  Reads what run_backward left at p.dvf and VisualProjection's weight as the parameter bucket holds
// it; allocates nothing, so a plan never sees this launch.
void run_input_grads(Ctx& c, float* d_video_features) {
    const Plan& p = *c.p;
    LAUNCH("vproj_dx", launch_vproj_dx(VprojDxArgs{c.W(p.dvf), c.P(c.h->P.va_w), d_video_features, p.NV() * p.T, c.h->cfg.video_feature_dim,
                                                   c.drop(SITE_VIS), c.h->cus}, c.s));
}

}  // namespace vsl
