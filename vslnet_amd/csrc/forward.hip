// The forward launch sequences: one encoder application, the rnn head's helpers, the stages (video branch, query branch, fusion + predictor)
// and the forwards composed from them.
#include "host.hpp"

namespace vsl {

struct HeadTail { HeadArgs hs, he; const float *x, *vmask; };     // AttnBlockArgs::head_tail
// `out`: where the application's output goes when that is not the plan's own buffer (vsl_encode_video: the caller's encoding)
static void enc_fwd(Ctx& c, const EncP& P, const EncPk& K, const EncWs& w, const float* xin, const float* mask, int Bn, int app, const HeadTail* ht = nullptr, float* out = nullptr) {
    const int R = w.R, L = w.L, H = c.h->cfg.num_heads;
    float* const yout = out ? out : c.W(w.out);
    {
        // the whole conv block + LN1 / QKV in ONE launch (kernels_enc.hip: 12-row recomputed halo)
        CbFwdArgs a;
        memset(&a, 0, sizeof a);
        a.xin = xin; a.pos = c.P(P.pos); a.x0_out = c.SV(w.x0); a.nosave = c.inf();
        for (int i = 0; i < 4; ++i) {
            a.ln_g[i] = c.P(P.lng[i]); a.ln_b[i] = c.P(P.lnb[i]); a.dw_w[i] = c.P(P.dw[i]);
            a.pw_b[i] = c.P(P.pwb[i]); a.y[i] = i == 3 ? c.W(w.y[i]) : c.SV(w.y[i]); a.u[i] = c.SV(w.u[i]);      // (y[3]: the attention block's residual input)
            a.relu_mask[i] = reinterpret_cast<uint32_t*>(c.SV(w.mask[i])); a.dp[i] = c.drop(app * 16 + i);
        }
        a.qf = QkvFuse{c.P(P.ln1g), c.P(P.ln1b), c.P(P.qb), c.P(P.kb), c.P(P.vb), c.SV(w.h1), c.W(w.q), c.W(w.k), c.W(w.v),
                       c.drop(app * 16 + 4)};
        for (int i = 0; i < 4; ++i) a.W3[i] = reinterpret_cast<const uint16_t*>(c.PK(K.pw_f3[i]));
        a.Wqkv3 = reinterpret_cast<const uint16_t*>(c.PK(K.qkv_f3));
        a.R = R; a.L = L;
        LAUNCH("convblock_fwd", launch_convblock_fwd(a, c.s));
    }
    if (H == 8 && L <= 128) {      // attention core + output block in one launch (kernels_enc.hip)
        AttnBlockArgs ab{c.W(w.q), c.W(w.k), c.W(w.v), mask, c.W(w.y[3]), c.P(P.ln2g), c.P(P.ln2b), c.PK(K.o_f), c.P(P.ob),
                         c.SV(w.att), c.SV(w.lse), c.SV(w.r), c.SV(w.h2), yout, L, 0,
                         c.drop(app * 16 + 5), c.drop(app * 16 + 6), c.drop(app * 16 + 7), c.drop(app * 16 + 8)};
        ab.nosave = c.inf();
        if (ht) { ab.head_tail = 1; ab.hs = ht->hs; ab.he = ht->he; ab.head_x = ht->x; ab.head_vmask = ht->vmask; }
        LAUNCH("attn_block_fwd", launch_attn_block_fwd(ab, Bn, c.s));
        return;
    }
    // every other head count, and longer sequences (K / V staged in LDS per 64 queries): the attention core, then the output block
    LAUNCH("attn_fwd", launch_attn_fwd(AttnArgs{c.W(w.q), c.W(w.k), c.W(w.v), mask, c.W(w.att), c.SV(w.lse), nullptr, nullptr, nullptr, nullptr, Bn, L, H, 0,
                                                c.drop(app * 16 + 5), Drop{}}, c.s));
    LAUNCH("attn_out_fwd", launch_attn_out_fwd(AttnOutFwdArgs{c.W(w.att), c.W(w.y[3]), c.P(P.ln2g), c.P(P.ln2b), c.PK(K.o_f), c.P(P.ob), c.SV(w.r), c.SV(w.h2), yout,
                                                              c.drop(app * 16 + 6), c.drop(app * 16 + 7), c.drop(app * 16 + 8)}, R, c.s));
}

static CharConvPtrs char_ptrs(const Ctx& c) {
    CharConvPtrs cc;
    for (int i = 0; i < 4; ++i) { cc.w[i] = c.P(c.h->P.ccw[i]); cc.b[i] = c.P(c.h->P.ccb[i]); }
    return cc;
}

// Time chunks of the rnn head's CHUNKED launches (batches the one-launch pipeline of kernels_lstm.hip does not take: 80 < B <= 256 and the
// 4-sample groups beyond; lengths in processing order): n equal chunks.  The second LSTM lags the first by one chunk and every chunk boundary is a
// cross-stream hop (~10-15 us on the chain: a stream that is already blocked on an event wakes up late), so n ~ sqrt(0.06 T): 3 chunks at
// T = 128, 4 at T = 256.  With the round-4 step (0.6 us) the choice hardly matters any more -- ms per step at B = 16, T = 128 for 1 / 2 / 3 / 4 / 6
// chunks: 0.823, 0.816, 0.817, 0.831, 0.869 (profiles/r04_rnn_chunk_sweep.txt): the hops eat what the overlap gains, which is why small batches
// go through k_rnn_fwd / k_rnn_bwd instead.  Measured and dropped earlier (profiles/r04_notes.md section 7): a shorter last chunk, the start
// LSTM's own input projection chunked, the start LSTM's dx GEMM chunk by chunk on the third stream.
std::vector<int> lstm_chunks(int T) {
    const int n = std::max(1, (int)std::lround(std::sqrt(0.06 * T)));
    std::vector<int> out;
    for (int i = 0; i < n; ++i) out.push_back((T * (i + 1)) / n - (T * i) / n);
    return out;
}

// Tag of one fused rnn launch's granules: unique per process and a NaN pattern (quiet NaN with a payload no arithmetic produces), so that
// nothing the caller's workspace may hold from earlier use -- activations, indices, older granules -- reads as a valid tag.
// The counter has 21 bits: after 2^21 fused launches (two per training step) the tags repeat.  `gen` = how often it has wrapped; a plan's granule
// buffers are cleared once per (workspace, generation) before a launch (rnn_granules_fresh), so a tag of generation g - 1 can never be read as
// one of generation g.  What remains an assumption: inside one generation the caller does not write its own data into the workspace range the
// plan uses for granules (include/vslnet_hip.h: the workspace belongs to the library between vsl_forward and vsl_backward of a step; across
// steps only its granule ranges must be left alone or be re-zeroed by a plan change).
std::atomic<unsigned long long> g_rnn_launches{0};
unsigned rnn_epoch(long long* gen) {
    // every tag carries the NaN pattern 0x7FE.....: counter value 0 gives 0x7FE00000, which is neither a cleared word (0) nor the tag of
    // the launch before or after it -- no remap (mapping it onto ...01 made it collide with the next launch's tag)
    const unsigned long long n = g_rnn_launches.fetch_add(1) + 1;
    if (gen) *gen = (long long)(n >> 21);
    return 0x7FE00000u | (unsigned)(n & 0x1FFFFFu);
}

// first use of a plan's granule buffers in this workspace, or the epoch counter has wrapped since: one memset on the launch stream
void rnn_granules_fresh(Ctx& c, Plan& p, long long gen) {
    for (const Plan::GranSeen& g : p.gran_seen)
        if (g.ws == (const void*)c.ws && g.gen == gen) return;
    (void)hipMemsetAsync(c.W(p.h_gran), 0, (size_t)p.gran_floats * sizeof(float), c.s);
    p.gran_seen[p.gran_next] = Plan::GranSeen{c.ws, gen};
    p.gran_next = (p.gran_next + 1) & 3;
}

// Lq <= 32: the query branch runs as sample-local launches (kernels_query.hip) in both directions (VSL_QUERY_FUSED=0: row-tile launches)
bool query_fused(const Ctx& c) {
    static const bool on = switch_on("VSL_QUERY_FUSED", true);
    return on && query_fused_ok(c.p->Lq, c.h->cfg.num_heads, c.h->cfg.word_dim + 100);
}

// ---- the stages: each enqueues on c.s and reads nothing but its arguments, the plan and the call's vsl_io

// VisualProjection of the call's features (fp32, or bf16: the throughput mode) over `rows` feature rows into `dst`
static void vproj_fwd(Ctx& c, float* dst, int rows) {
    const vsl_config& cf = c.h->cfg; const ModelP& P = c.h->P; const ModelPk& K = c.h->K;
    const vsl_io& io = *c.io;
    if (io.video_features_bf16)
        LAUNCH("vproj_fwd", launch_vproj_fwd_bf16(io.video_features_bf16, reinterpret_cast<const uint16_t*>(c.PK(K.va_f16)), c.P(P.va_b), dst, rows,
                                                  cf.video_feature_dim, c.drop(SITE_VIS), c.s));
    else
        LAUNCH("vproj_fwd", launch_vproj_fwd3(io.video_features, reinterpret_cast<const uint16_t*>(c.PK(K.va_f3)), c.P(P.va_b), dst, rows, cf.video_feature_dim,
                                              c.drop(SITE_VIS), c.s));
}

// jobs first .. first + n - 1 of the handle's pack table: the matrix-core operands of the call's parameters into the plan's pack area
static void pack_jobs(Ctx& c, int first, int n) {
    LAUNCH("pack", launch_pack(c.io->params, c.W(c.p->pack), c.h->jobs_dev + first, n, c.s));
}

// VisualProjection + encoder application 0 over the clips of the plan's video half (B x T; N x T in a shared training step); `out`: the caller's encoding (vsl_encode_video), nullptr = the plan's own buffer
static void video_branch(Ctx& c, float* out) {
    const Plan& p = *c.p;
    const int Nv = p.NV();
    vproj_fwd(c, c.W(p.vf), Nv * p.T);
    enc_fwd(c, c.h->P.fe, c.h->K.fe, p.ve, c.W(p.vf), c.video_mask(), Nv, 0, nullptr, out);
}

// a pack launch another stream's kernel has to wait for: its stop event and its record in the profiler's ledger (nullptr / -1: nothing to wait for)
struct PackWait { hipEvent_t ev = nullptr; int rec = -1; };

// word + char embedding, then the Embedding linear + encoder application 1; `emb_pack`: the Embedding linear's operand when another stream packs it;
// `out`: the caller's encoding (vsl_encode_query), nullptr = the plan's own buffer
static void query_branch(Ctx& c, PackWait emb_pack, float* out = nullptr) {
    const vsl_config& cf = c.h->cfg; const ModelP& P = c.h->P; const ModelPk& K = c.h->K;
    const Plan& p = *c.p; const vsl_io& io = *c.io;
    const int B = p.B, Lq = p.Lq, Rq = B * Lq;
    const bool wt = cf.word_table != 0;       // trainable word table: its rows 0, 1, 2.. are pad, unk, the vocabulary
    const float* tab = c.P(P.unk);            // (word table: P.unk is its first row)
    LAUNCH("embed_fwd", launch_embed_fwd(EmbedFwdArgs{io.word_ids, io.char_ids, wt ? tab : io.pad_vec, tab + (wt ? cf.word_dim : 0), wt ? tab + 2 * cf.word_dim : io.glove_vec,
                                                      c.P(P.char_tab), char_ptrs(c), c.PK(K.ccw_img), c.W(p.E), reinterpret_cast<int8_t*>(c.SV(p.argpos)), Rq, p.Lc,
                                                      cf.word_dim, cf.char_dim, c.drop(SITE_WORD), c.drop(SITE_CHAR)}, c.s));
    if (emb_pack.ev) {                // behind embed_fwd, which reads the char-conv image alone
        (void)hipStreamWaitEvent(c.s, emb_pack.ev, 0); c.h->mark_waiting(c.s);
        if (emb_pack.rec >= 0) c.h->prof_pending.push_back({c.s, emb_pack.rec});
    }
    if (query_fused(c)) {
        // the rest of the query branch in ONE sample-local launch (kernels_query.hip)
        QueryFwdArgs qa;
        memset(&qa, 0, sizeof qa);
        const EncP& E = P.fe; const EncPk& EK = K.fe; const EncWs& w = p.qe;
        qa.E = c.W(p.E); qa.Wemb3 = reinterpret_cast<const uint16_t*>(c.PK(K.emb_f3)); qa.b_emb = c.P(P.emb_b); qa.qf = c.SV(p.qf); qa.nosave = c.inf();
        qa.pos = c.P(E.pos); qa.x0 = c.SV(w.x0);
        for (int i = 0; i < 4; ++i) {
            qa.W3[i] = reinterpret_cast<const uint16_t*>(c.PK(EK.pw_f3[i]));
            qa.ln_g[i] = c.P(E.lng[i]); qa.ln_b[i] = c.P(E.lnb[i]); qa.dw_w[i] = c.P(E.dw[i]); qa.pw_b[i] = c.P(E.pwb[i]);
            qa.y[i] = c.SV(w.y[i]); qa.u[i] = c.SV(w.u[i]); qa.relu_mask[i] = reinterpret_cast<uint32_t*>(c.SV(w.mask[i])); qa.dp[i] = c.drop(16 + i);
        }
        qa.Wqkv3 = reinterpret_cast<const uint16_t*>(c.PK(EK.qkv_f3)); qa.Wo3 = reinterpret_cast<const uint16_t*>(c.PK(EK.o_f3));
        qa.ln1_g = c.P(E.ln1g); qa.ln1_b = c.P(E.ln1b); qa.bq = c.P(E.qb); qa.bk = c.P(E.kb); qa.bv = c.P(E.vb);
        qa.h1 = c.SV(w.h1); qa.q = c.SV(w.q); qa.k = c.SV(w.k); qa.v = c.SV(w.v); qa.d1 = c.drop(16 + 4);
        qa.mask = io.q_mask; qa.ln2_g = c.P(E.ln2g); qa.ln2_b = c.P(E.ln2b); qa.bo = c.P(E.ob);
        qa.att = c.SV(w.att); qa.lse = c.SV(w.lse); qa.r = c.SV(w.r); qa.h2 = c.SV(w.h2); qa.out = out ? out : c.W(w.out);
        qa.d2 = c.drop(16 + 5); qa.d3 = c.drop(16 + 6); qa.d4 = c.drop(16 + 7); qa.d5 = c.drop(16 + 8);
        qa.EW = cf.word_dim + 100; qa.L = Lq; qa.b_off = 0;
        LAUNCH("query_fwd", launch_query_fwd(qa, B, c.s));
        return;
    }
    if ((cf.word_dim + 100) % 16 == 0)
        LAUNCH("linear_fwd", launch_linear_fwd3(c.W(p.E), reinterpret_cast<const uint16_t*>(c.PK(K.emb_f3)), c.P(P.emb_b), c.W(p.qf), Rq, cf.word_dim + 100, c.s));
    else          // a width the 16-wide K steps of the split kernel do not tile: the fp32-input MFMA kernel (K streamed in chunks)
        LAUNCH("linear_fwd", launch_linear_fwd(c.W(p.E), c.PK(K.emb_f), c.P(P.emb_b), c.W(p.qf), Rq, cf.word_dim + 100, c.s));
    enc_fwd(c, P.fe, K.fe, p.qe, c.W(p.qf), io.q_mask, B, 1, nullptr, out);
}

// CQAttention, CQConcatenate and the highlight layer: h_score is final behind cq_out, which also leaves `gated` for the predictor
static void cq_and_highlight(Ctx& c, CqContext ctx) {
    const ModelP& P = c.h->P; const ModelPk& K = c.h->K;
    const Plan& p = *c.p; const vsl_io& io = *c.io;
    const int B = p.B, T = p.T, Lq = p.Lq;
    // short videos, short queries: the column kernel (column softmax over the clips, M = S_col^T C, WeightedPool) is folded into its neighbours --
    // one launch and one boundary less on the dependent chain (VSL_CQ_FOLD=0: three launches)
    static const bool fold_on = switch_on("VSL_CQ_FOLD", true);
    const bool cq_fold = fold_on && cq_col_folds(T, Lq);
    CqFwdArgs cq;
    cq.C = ctx.C; cq.vidx = ctx.vidx; cq.vmask = io.v_mask;
    cq.Qf = ctx.Qf ? ctx.Qf : c.W(p.qe.out); cq.qmask = ctx.Qf ? ctx.qmask : io.q_mask; cq.qidx = ctx.Qf ? ctx.qidx : nullptr;
    cq.w4C = c.P(P.w4C); cq.w4Q = c.P(P.w4Q); cq.w4mlu = c.P(P.w4mlu);
    cq.S = c.W(p.S); cq.Srow = c.W(p.Srow); cq.Scol = c.SV(p.Scol);
    cq.Mpart = c.W(p.cqP1); cq.M = c.SV(p.M);       // the per-tile partials of M go where the backward's cqP1 arena is free until then
    cq.pool = CqPoolArgs{c.P(P.pool_w), c.P(P.cat_w), c.P(P.cat_b), c.SV(p.alpha), c.SV(p.pooled), c.W(p.pb)};
    cq.Wcqa = c.PK(K.cqa_f); cq.bcqa = c.P(P.cqa_b); cq.W1pack = c.PK(K.cat1_f); cq.wh = c.P(P.hl_w); cq.bh = c.P(P.hl_b);
    cq.cat = c.SV(p.cat); cq.f1 = c.SV(p.f1); cq.f2 = c.SV(p.f2); cq.hscore = io.h_score; cq.gated = c.W(p.gated);
    cq.B = B; cq.T = T; cq.Lq = Lq; cq.b_off = 0; cq.dc = c.drop(SITE_CQ_C); cq.dq = c.drop(SITE_CQ_Q); cq.fold = cq_fold;
    LAUNCH("cq_score", launch_cq_score(cq, c.s));
    if (!cq_fold) LAUNCH("cq_col", launch_cq_col(cq, c.s));
    // cq_out also carries CQConcatenate + HighLightLayer + gating (row-local on the tile it produces)
    LAUNCH("cq_out", launch_cq_out(cq, c.s));
}

// CQAttention over the context and the encoded query, CQConcatenate, the highlight score, the predictor and the span heads -- the dependent chain
// behind the join of the two branches
static void fuse_and_predict(Ctx& c, CqContext ctx) {
    const vsl_config& cf = c.h->cfg; const ModelP& P = c.h->P; const ModelPk& K = c.h->K;
    const Plan& p = *c.p; const vsl_io& io = *c.io;
    const int B = p.B, T = p.T, R = B * T;
    hipStream_t sq = c.side(0);
    cq_and_highlight(c, ctx);
    if (cf.predictor == 0) {
        // rnn head (:341-343): start = LSTM_s(x) * mask ; end = LSTM_e(start) * mask ; no LayerNorm in front of the span blocks
        // The recurrence is latency bound (one sample per CU, 0.6 us per step).  Up to RNN_FUSED_MAX_B samples the whole head is ONE launch: start
        // LSTM, input projection and end LSTM as three workgroups per sample that hand each step over in-launch (k_rnn_fwd).  Larger batches
        // pipeline the two LSTMs in TIME CHUNKS over three streams: while the start LSTM runs chunk k + 1 on the main stream, a side stream
        // projects its chunk k (x W_ih^T of the end LSTM, a row-mapped GEMM) and another runs the end LSTM over it.  A chunk launch resumes from
        // the state the previous one saved for the backward (h_{t-1}, c_{t-1}).  Chunking: lstm_chunks().
        const std::vector<int> chunks = lstm_chunks(T);
        auto lstm = [&](int l, int t0, int t1) {
            const LstmWs& w = p.lstm[l];
            LAUNCH("lstm_fwd", launch_lstm_fwd(c.W(w.gi), c.P(P.l_whh[l]), c.PK(K.l_hf[l]), c.P(P.l_bih[l]), c.P(P.l_bhh[l]), io.v_mask, c.SV(w.gates),
                                               c.W(w.cseq), c.SV(w.tseq), c.W(w.hprev), c.W(w.out), B, T, c.s, t0, t1));      // (cseq, hprev: a later chunk resumes from them)
        };
        // gate projections gi = x W_ih^T: (rows,128) x (128,512), no bias, bf16x6 on the matrix cores
        auto gi = [&](int l, const float* x, int rows, int seg = 0, int off = 0) {
            LAUNCH("lstm_gi", launch_linear_fwd3(x, reinterpret_cast<const uint16_t*>(c.PK(K.l_f3[l])), nullptr, c.W(p.lstm[l].gi), rows, D, c.s, 4 * D, seg, T, off));
        };
        gi(0, c.W(p.gated), R);
        hipStream_t main_s = c.s;
        if (p.h_gran >= 0) {
            // one launch, three workgroups per sample (kernels_lstm.hip: k_rnn_fwd)
            RnnFwdArgs a;
            memset(&a, 0, sizeof a);
            a.gi0 = c.W(p.lstm[0].gi); a.Wih1 = c.PK(K.l_if); a.mask = io.v_mask;
            for (int l = 0; l < 2; ++l) {
                const LstmWs& w = p.lstm[l];
                a.Whh[l] = c.PK(K.l_hf[l]); a.bih[l] = c.P(P.l_bih[l]); a.bhh[l] = c.P(P.l_bhh[l]);
                a.gates[l] = c.SV(w.gates); a.cseq[l] = c.SV(w.cseq); a.tseq[l] = c.SV(w.tseq); a.hprev[l] = c.SV(w.hprev); a.out[l] = c.W(w.out);
            }
            a.h_gran = reinterpret_cast<unsigned long long*>(c.W(p.h_gran)); a.gi_gran = reinterpret_cast<unsigned long long*>(c.W(p.gi_gran));
            long long gen = 0;
            a.epoch = rnn_epoch(&gen); a.B = B; a.T = T; a.nosave = c.inf();
            rnn_granules_fresh(c, *c.p, gen);
            LAUNCH("rnn_fwd", launch_rnn_fwd(a, c.s));
        } else if (chunks.size() < 2 || sq == main_s) {
            lstm(0, 0, T);
            gi(1, c.W(p.lstm[0].out), R);
            lstm(1, 0, T);
        } else {
            // Three streams (round 4): the end LSTM's input projection of chunk k (a 15 us GEMM) runs on the third stream behind the start
            // LSTM's chunk k, BESIDE the end LSTM's chunk k - 1 -- on the end LSTM's own stream it made that chain 59 us per chunk against 39
            // for the start LSTM, and the end LSTM finished 144 us after the start LSTM (profiles/r04_notes.md section 7).
            hipStream_t sg = c.side(1) != main_s ? c.side(1) : sq;
            int t0 = 0;
            for (int len : chunks) {
                const int t1 = t0 + len;
                lstm(0, t0, t1);
                c.order(main_s, sg);
                c.s = sg;
                gi(1, c.W(p.lstm[0].out), B * (t1 - t0), t1 - t0, t0);
                c.order(sg, sq);
                c.s = sq;
                lstm(1, t0, t1);
                c.s = main_s;
                t0 = t1;
            }
            c.order(sq, main_s);
        }
        HeadArgs hs{c.W(p.lstm[0].out), nullptr, nullptr, c.PK(K.s0_f), c.P(P.s0b), c.P(P.s1w), c.P(P.s1b), c.SV(p.hid_s), nullptr, io.start_logits};
        HeadArgs he{c.W(p.lstm[1].out), nullptr, nullptr, c.PK(K.e0_f), c.P(P.e0b), c.P(P.e1w), c.P(P.e1b), c.SV(p.hid_e), nullptr, io.end_logits};
        LAUNCH("head_fwd", launch_head_fwd(hs, he, c.W(p.gated), io.v_mask, R, c.s));
        return;
    }
    enc_fwd(c, P.pe, K.pe, p.p1, c.W(p.gated), io.v_mask, B, 2);
    HeadArgs hs{c.W(p.p1.out), c.P(P.sln_g), c.P(P.sln_b), c.PK(K.s0_f), c.P(P.s0b), c.P(P.s1w), c.P(P.s1b), c.SV(p.hid_s),
                c.SV(p.lnf_s), io.start_logits};
    HeadArgs he{c.W(p.p2.out), c.P(P.eln_g), c.P(P.eln_b), c.PK(K.e0_f), c.P(P.e0b), c.P(P.e1w), c.P(P.e1b), c.SV(p.hid_e),
                c.SV(p.lnf_e), io.end_logits};
    // T <= 128: the second pass' attention-block kernel goes on with both span heads on its tiles (one launch less on the dependent chain)
    static const bool heads_on = switch_on("VSL_HEADS_FUSED", true);
    const bool heads_hosted = heads_on && cf.num_heads == 8 && attn_block_fwd_hosts_heads(T);
    HeadTail ht{hs, he, c.W(p.gated), io.v_mask};
    enc_fwd(c, P.pe, K.pe, p.p2, c.W(p.p1.out), io.v_mask, B, 3, heads_hosted ? &ht : nullptr);
    if (!heads_hosted) LAUNCH("head_fwd", launch_head_fwd(hs, he, c.W(p.gated), io.v_mask, R, c.s));
}

// ---- the forwards: which packs go where, what forks and what joins

// The third stream's pack launches: the Embedding linear's operand first (the query branch waits for it behind embed_fwd: the returned PackWait),
// then everything the two branches do not read.  The caller has made `sp` wait for whatever has to come first.
static PackWait side_packs(Ctx& c, hipStream_t sp) {
    const vsl_handle_s* h = c.h;
    const int nj = (int)h->jobs.size(), head = h->jobs_char + h->jobs_first, nj1 = h->jobs_query;
    hipStream_t keep = c.s;
    c.s = sp;
    pack_jobs(c, head, nj1);
    PackWait w;
    w.ev = h->last_event(sp);
    w.rec = h->prof_on ? (int)h->prof_recs.size() - 1 : -1;
    pack_jobs(c, head + nj1, nj - head - nj1);
    c.s = keep;
    return w;
}

// vsl_forward / vsl_forward_shared: the video branch and the query branch side by side, joined in front of the CQ kernels.  `vidx` (a shared training
// step: c.sh set, plan TrainShared, N videos, B queries, query b against video video_index[b]): the video branch ran over
// the plan's N videos and CQAttention reads its output through the index; the grouping of the queries by video (the backward's reduction of dC reads
// it) is built beside the branches on the pack stream, off the dependent chain
void forward_full(Ctx& c) {
    const int* const vidx = c.video_index();
    const vsl_handle_s* h = c.h;
    const Plan& p = *c.p;
    const int nj = (int)h->jobs.size(), nfirst = h->jobs_char + h->jobs_first;
    hipStream_t sq = c.side(0), sp = c.side(1);
    const bool split3 = sq != c.main && sp != c.main;
    PackWait emb_pack;
    if (split3) {
        // The main stream's pack carries the char-conv image as well, so the query stream's first kernel -- the word + char embedding, 160
        // workgroups x 125 KB of LDS -- starts right behind it and runs beside the remaining packs and VisualProjection, not beside the video
        // pass' conv block (which it kept off 160 CUs: 49 us in the step against 25 alone, profiles/r05_notes.md section 9); the Embedding
        // linear's operand is packed on the third stream meanwhile.
        pack_jobs(c, 0, nfirst);
        c.order2(c.main, sq, sp);
        emb_pack = side_packs(c, sp);
    } else {
        pack_jobs(c, 0, nj);
        c.order(c.main, sq);        // fork: the query branch (embedding + query encoder pass) runs beside the video branch
    }
    // The video branch (VisualProjection 19 + conv block 35 + attention 24 us) and the query branch (embedding 30 + linear 17 +
    // conv block 25 + attention 11) are about even at the headline shape; the main stream keeps the video branch (swap: +0.6 %).
    video_branch(c, nullptr);
    c.s = sq;
    query_branch(c, emb_pack);
    c.s = c.main;
    c.order(sq, c.main);                   // join
    if (vidx) {
        int* const csr = reinterpret_cast<int*>(c.W(p.csr));
        c.s = split3 ? sp : c.main;
        LAUNCH("group_csr", launch_group_csr(vidx, p.B, p.NV(), csr, csr + p.csr_members(), c.s));
        c.s = c.main;
    }
    if (split3) c.order(sp, c.main);       // the remaining packs (long done)
    fuse_and_predict(c, CqContext{c.W(p.ve.out), vidx});
}

// vsl_encode_video: the video half alone -- the shared encoder's and VisualProjection's operands, the projection, encoder application 0
// into the caller's buffer.  One stream: there is no query branch to run beside it.
void forward_encode(Ctx& c, float* video_encoding) {
    pack_jobs(c, c.h->jobs_char, c.h->jobs_first);
    video_branch(c, video_encoding);
}

// vsl_encode_windows: the pack of forward_encode, VisualProjection ONCE over the call's feature rows into the plan's (rows, 128) buffer, the gather of
// every window's rows (and of the projection of a zero row behind its length) into the slot the encoder reads, the (N, T) mask into the caller's
// buffer, then encoder application 0 over the windows into the caller's encoding.  One stream, as forward_encode.
void forward_encode_windows(Ctx& c, const int32_t* window_row, const int32_t* window_len, float* v_mask, float* video_encoding) {
    const ModelP& P = c.h->P;
    const Plan& p = *c.p;
    pack_jobs(c, c.h->jobs_char, c.h->jobs_first);
    vproj_fwd(c, c.W(p.wproj), p.rows);
    LAUNCH("window_gather", launch_window_gather(WindowGatherArgs{c.W(p.wproj), c.P(P.va_b), window_row, window_len, c.W(p.vf), v_mask, p.B, p.T, p.rows}, c.s));
    enc_fwd(c, P.fe, c.h->K.fe, p.ve, c.W(p.vf), v_mask, p.B, 0, nullptr, video_encoding);
}

// vsl_encode_query: the query half alone into the caller's buffer -- the char-conv image and the shared encoder's operands (the head of the first
// class: VisualProjection's, its last jobs_va jobs, stay unpacked), the Embedding linear's operand, then the query branch.  One stream: there is
// nothing to run beside it.
void forward_encode_query(Ctx& c, float* query_encoding) {
    const vsl_handle_s* h = c.h;
    const int head = h->jobs_char + h->jobs_first;
    pack_jobs(c, 0, head - h->jobs_va);
    pack_jobs(c, head, h->jobs_query);
    query_branch(c, PackWait{}, query_encoding);
}

// vsl_localize: the query branch is the ONLY chain in front of the CQ kernels, so it owns the main stream and there is no fork and no join on the
// dependent chain (each costs a ~6 - 20 us bubble, see Ctx::order_n); the packs it does not read and the mask gather run beside it on the third stream.
// VisualProjection's operands -- the last jobs_va jobs of the first class, the largest pack job -- stay unpacked.
void forward_localize(Ctx& c, CqContext ctx, const float* vmask_nt) {
    const vsl_handle_s* h = c.h;
    const Plan& p = *c.p;
    const int nj = (int)h->jobs.size(), head = h->jobs_char + h->jobs_first, nfirst = head - h->jobs_va;
    hipStream_t sp = c.side(1);
    const bool split3 = c.side(0) != c.main && sp != c.main;
    PackWait emb_pack;
    pack_jobs(c, 0, nfirst);
    if (split3) {
        c.order(c.main, sp);
        emb_pack = side_packs(c, sp);
        c.s = sp;
    } else {
        pack_jobs(c, head, nj - head);
    }
    // the per-query clip mask, beside the query branch; first read by the CQ kernels, behind the join with its stream
    LAUNCH("vmask_gather", launch_vmask_gather(vmask_nt, ctx.vidx, c.W(p.vmask), p.B, p.T, c.s));
    c.s = c.main;
    query_branch(c, emb_pack);
    if (split3) c.order(sp, c.main);       // the remaining packs (long done) and the gathered mask
    fuse_and_predict(c, ctx);
}

// vsl_localize_pairs: no query branch at all -- both sides of CQAttention are resident encodings read through their indices.  Only the "rest" class of
// packs is needed (no char image, no shared-encoder, Embedding or VisualProjection operands); the mask gather runs beside it on the third stream.
// (pairs_pack_and_mask: everything of it in front of the CQ kernels; vsl_highlight_pairs starts the same way)
static void pairs_pack_and_mask(Ctx& c, CqContext ctx, const float* vmask_nt) {
    const vsl_handle_s* h = c.h;
    const Plan& p = *c.p;
    const int nj = (int)h->jobs.size(), rest = h->jobs_char + h->jobs_first + h->jobs_query;
    hipStream_t sp = c.side(1);
    const bool split = sp != c.main;
    if (split) { c.order(c.main, sp); c.s = sp; }      // (behind whatever the caller's stream holds: the workspace may still be read by an earlier call)
    // the per-pair clip mask, beside the pack; first read by the CQ kernels, behind the join with its stream
    LAUNCH("vmask_gather", launch_vmask_gather(vmask_nt, ctx.vidx, c.W(p.vmask), p.B, p.T, c.s));
    c.s = c.main;
    pack_jobs(c, rest, nj - rest);
    if (split) c.order(sp, c.main);
}

void forward_pairs(Ctx& c, CqContext ctx, const float* vmask_nt) {
    pairs_pack_and_mask(c, ctx, vmask_nt);
    fuse_and_predict(c, ctx);
}

// vsl_highlight_pairs: what forward_pairs enqueues up to cq_out -- the same kernels in the same order, so h_score holds the bits vsl_localize_pairs
// gives -- then one launch that reduces every pair's row to its relevance.  No predictor, no span heads.
void forward_highlight(Ctx& c, CqContext ctx, const float* vmask_nt, float* out, int ld, int mean) {
    pairs_pack_and_mask(c, ctx, vmask_nt);
    cq_and_highlight(c, ctx);
    LAUNCH("pair_relevance", launch_pair_relevance(RelevanceArgs{c.io->h_score, c.io->v_mask, ctx.vidx, ctx.qidx, out, c.p->B, c.p->T, ld, mean}, c.s));
}

}  // namespace vsl
