// Per-shape plans: the workspace layout of each plan kind, the reduction tables of the training plan, and the plan cache.
#include "host.hpp"

namespace vsl {

namespace {

struct Bump {
    int64_t cur = 0;
    int64_t operator()(int64_t n) { const int64_t o = cur; cur += (n + 3) & ~int64_t(3); return o; }
};
void plan_encoder(Bump& al, EncWs& w, int Bn, int L, int H) {
    const int64_t R = (int64_t)Bn * L;
    w.R = (int)R; w.L = L;
    w.x0 = al(R * D);
    for (int i = 0; i < 4; ++i) { w.y[i] = al(R * D); w.u[i] = al(R * D); w.mask[i] = al(R * 4); }
    w.h1 = al(R * D); w.q = al(R * D); w.k = al(R * D); w.v = al(R * D);
    w.lse = al((int64_t)Bn * H * L);
    w.att = al(R * D); w.r = al(R * D); w.h2 = al(R * D); w.out = al(R * D);
}

// the limits of the video side: a row of the positional table per clip, the attention kernels' longest sequence, and 32-bit byte offsets into (R, 128)
// tensors in the conv-block kernels (0x80000000 marks a dropped lane).  `what`: hint appended to the row-limit message
int check_video_shape(vsl_handle_s* h, int N, int T, const char* what) {
    const vsl_config& cf = h->cfg;
    if (T > cf.max_pos_len)
        return fail("sequence length (T=%d) exceeds max_pos_len=%d: the positional table has no such row (layers_t7.py:196 -- IndexError in the reference)", T, cf.max_pos_len);
    if (T > MAX_L) return fail("T=%d > %d clips not supported by the attention kernels", T, MAX_L);
    if ((int64_t)N * T * D * 4 >= (int64_t(1) << 31))
        return fail("B*T = %lld rows: an (R, 128) fp32 activation must stay below 2 GiB for the 32-bit buffer offsets of the conv-block kernels%s", (long long)N * T, what);
    return 0;
}

// limits of a shape that are about addressing, not about the size of a plan (every plan kind with a query side)
int check_shape(vsl_handle_s* h, int B, int T, int Lq, int Lc) {
    const vsl_config& cf = h->cfg;
    if (B <= 0 || T <= 0 || Lq <= 0) return fail("empty batch (B=%d T=%d Lq=%d)", B, T, Lq);
    if (int rc = check_video_shape(h, B, T, "")) return rc;
    if (Lq > cf.max_pos_len)
        return fail("sequence length (Lq=%d) exceeds max_pos_len=%d: the positional table has no such row (layers_t7.py:196 -- IndexError in the reference)", Lq, cf.max_pos_len);
    if (Lq > MAX_LQ) return fail("Lq=%d > %d query words: the CQAttention kernels keep the whole query of a sample in LDS "
                                 "(the reference truncates at max_pos_len words, data_gen.py:188)", Lq, MAX_LQ);
    if ((int64_t)B * Lq * D * 4 >= (int64_t(1) << 31))
        return fail("B*Lq = %lld rows: an (R, 128) fp32 activation must stay below 2 GiB for the 32-bit buffer offsets of the conv-block kernels", (long long)B * Lq);
    if (Lc < 4 || Lc > MAX_LC) return fail("Lc=%d must be in [4, %d] (the widest char conv has kernel 4, layers_t7.py:52)", Lc, MAX_LC);
    if (cf.predictor == 0 && (int64_t)B * T * 4 * D >= (int64_t(1) << 31)) return fail("B*T = %lld too large for the 32-bit offsets of the LSTM kernels", (long long)B * T);
    return 0;
}

// the scratch of ONE encoder application in a forward-only plan: five (R, 128) slots y3, q, k, v, att from `region` on (RD floats each)
void place_encoder(EncWs& w, int64_t region, int64_t RD) {
    w.y[3] = region; w.q = region + RD; w.k = region + 2 * RD; w.v = region + 3 * RD; w.att = region + 4 * RD;
}

// The inference plan (vsl_io.inference): what a forward keeps live and nothing else -- no saves, no backward temporaries, no partial arena, no
// reduction tables.  Buffers are reused by liveness along the main stream's order (forward_full):
//   region : y3, q, k, v, att of ONE encoder application -- the video pass, then both predictor passes; VisualProjection's output (dead once the
//            video pass' conv block has run) sits in the att slot; between the video pass and the predictor the same floats hold the CQ kernels'
//            S, Srow and the per-tile partials of M (the region is as large as the larger of the two uses); rnn: the start LSTM's gate projection
//   a      : the video encoder's output, dead behind cq_out -> the second predictor pass' / the end LSTM's output
//   gated, p1.out : live up to the span heads
// The query branch runs beside the video pass on its own stream and has its own (B Lq)-row scratch.  The rnn head keeps the second gate projection
// and its hand-off granules (B <= 80) or, for the chunked launches, the c_t / h_t sequences a later time chunk resumes from.
// Every offset a forward does not use stays -1 (Ctx::SV hands the kernels nullptr for those).
// PlanKind::Localize (vsl_localize): the same plan without a video pass -- the context is the caller's resident encoding, so `a` serves the second predictor
// pass / the end LSTM alone and nothing here ever holds a (B, T, 128) copy of the encoding; the (B, T) gathered clip mask is added and vsl_loss's
// scratch (there is no vsl_io to call it with) left out, so the plan never exceeds the inference plan of the shape by more than B T floats.
// PlanKind::LocalizePairs (vsl_localize_pairs): the Localize plan without the query branch's scratch -- the encoded queries are resident too.
int build_infer_plan(vsl_handle_s* h, int B, int T, int Lq, int Lc, Plan** out, PlanKind kind) {
    if (int rc = check_shape(h, B, T, Lq, Lc)) return rc;
    const vsl_config& cf = h->cfg;
    const bool video = kind != PlanKind::Localize && kind != PlanKind::LocalizePairs;
    const bool query = kind != PlanKind::LocalizePairs;          // (vsl_localize_pairs: the encoded queries are the caller's, there is no query branch)
    Plan* p = new Plan();
    p->kind = kind;
    p->B = B; p->T = T; p->Lq = Lq; p->Lc = Lc;
    const int64_t R = (int64_t)B * T, Rq = (int64_t)B * Lq, RD = ((R * D) + 3) & ~int64_t(3);
    const int EW = cf.word_dim + 100;
    for (EncWs* w : {&p->ve, &p->p1, &p->p2}) { w->R = (int)R; w->L = T; }
    p->qe.R = (int)Rq; p->qe.L = Lq;
    Bump al;
    p->pack = al(h->pack_floats);
    if (video) p->loss_scratch = al(5 * (int64_t)B + 8);          // (vsl_loss on the outputs of an inference forward)
    // the query branch's own scratch (beside the video pass on another stream)
    if (query) {
        p->E = al(Rq * EW); p->qf = al(Rq * D);
        p->qe.y[3] = al(Rq * D); p->qe.q = al(Rq * D); p->qe.k = al(Rq * D); p->qe.v = al(Rq * D); p->qe.att = al(Rq * D); p->qe.out = al(Rq * D);
    }
    p->pb = al((int64_t)B * D);
    // the region
    const int64_t nt = (T + TILE_M - 1) / TILE_M;
    const int64_t SL = ((R * Lq) + 3) & ~int64_t(3);
    const int64_t cq_need = 2 * SL + (((int64_t)B * nt * Lq * D + 3) & ~int64_t(3));
    const int64_t region = al(std::max(5 * RD, cq_need));
    if (video) { place_encoder(p->ve, region, RD); p->vf = p->ve.att; }
    place_encoder(p->p1, region, RD); place_encoder(p->p2, region, RD);
    p->S = region; p->Srow = region + SL; p->cqP1 = region + 2 * SL;
    const int64_t a = al(R * D);
    if (video) p->ve.out = a;
    p->gated = al(R * D);
    p->p1.out = al(R * D);
    p->p2.out = a;
    if (!video) p->vmask = al(R);
    if (cf.predictor == 0) {
        for (int l = 0; l < 2; ++l) {
            LstmWs& w = p->lstm[l];
            w.gi = l == 0 ? region : al(R * 4 * D);
            if (!rnn_fused_ok(B)) { w.cseq = al(R * D); w.hprev = al(R * D); }      // chunked launches: a chunk resumes from the last c_t, h_t of the one before
            w.out = l == 0 ? p->p1.out : p->p2.out;
        }
        if (rnn_fused_ok(B)) {
            p->h_gran = al(R * 2 * D); p->gi_gran = al(R * 8 * D);
            p->gran_floats = (p->gi_gran + R * 8 * D) - p->h_gran;      // the two allocations are consecutive
        }
    }
    p->partial = al(0);
    p->total = al.cur;
    if (p->total >= (int64_t(1) << 31)) { delete p; return fail("inference workspace of %lld floats exceeds the 2^31 offset range", (long long)p->total); }
    *out = p;
    return 0;
}

// vsl_encode_video: the operand packs and ONE encoder application's scratch (VisualProjection's output in the att slot, as in the inference plan).
// The output goes to the caller's buffer.  B = videos; the plan has no query side (Lq = Lc = 0 in its key).
int build_encode_plan(vsl_handle_s* h, int N, int T, Plan** out) {
    if (N < 1 || T < 1) return fail("vsl_encode_video: empty call (N=%d videos, T=%d clips)", N, T);
    if (int rc = check_video_shape(h, N, T, " (encode the videos in chunks)")) return rc;
    Plan* p = new Plan();
    p->kind = PlanKind::Encode;
    p->B = N; p->T = T; p->Lq = 0; p->Lc = 0;
    const int64_t R = (int64_t)N * T, RD = ((R * D) + 3) & ~int64_t(3);
    p->ve.R = (int)R; p->ve.L = T;
    Bump al;
    p->pack = al(h->pack_floats);
    place_encoder(p->ve, al(5 * RD), RD);
    p->vf = p->ve.att;
    p->partial = al(0);
    p->total = al.cur;
    if (p->total >= (int64_t(1) << 31)) { delete p; return fail("encode workspace of %lld floats exceeds the 2^31 offset range", (long long)p->total); }
    *out = p;
    return 0;
}

// vsl_encode_windows: the encode plan of (N windows, T) -- so the encoder application runs in the slots vsl_encode_video gives it -- plus the
// (rows, 128) projection of the feature rows behind it.  B = windows; rows sits in the key's N slot, Plan::N stays 0 (NV() = the windows).
int build_windows_plan(vsl_handle_s* h, int N, int T, int rows, Plan** out) {
    if (N < 1) return fail("vsl_encode_windows: N=%d windows (at least one)", N);
    if (T < 1 || T > std::min(MAX_L, h->cfg.max_pos_len))
        return fail("vsl_encode_windows: T=%d clips per window must be in [1, %d] (min of %d and max_pos_len=%d)", T, std::min(MAX_L, h->cfg.max_pos_len), MAX_L, h->cfg.max_pos_len);
    if (rows < 1) return fail("vsl_encode_windows: rows=%d feature rows (at least one)", rows);
    if ((int64_t)rows * h->cfg.video_feature_dim >= (int64_t(1) << 31))
        return fail("vsl_encode_windows: rows * video_feature_dim = %lld must stay below 2^31 (hand the call fewer feature rows)", (long long)rows * h->cfg.video_feature_dim);
    if ((int64_t)rows * D >= (int64_t(1) << 31)) return fail("vsl_encode_windows: rows * 128 = %lld must stay below 2^31 (hand the call fewer feature rows)", (long long)rows * D);
    if ((int64_t)N * T * D >= (int64_t(1) << 31)) return fail("vsl_encode_windows: N * T * 128 = %lld must stay below 2^31 (encode the windows in chunks)", (long long)N * T * D);
    if (int rc = check_video_shape(h, N, T, " (encode the windows in chunks)")) return rc;
    Plan* p = new Plan();
    p->kind = PlanKind::EncodeWindows;
    p->B = N; p->T = T; p->Lq = 0; p->Lc = 0; p->rows = rows;
    const int64_t R = (int64_t)N * T, RD = ((R * D) + 3) & ~int64_t(3);
    p->ve.R = (int)R; p->ve.L = T;
    Bump al;
    p->pack = al(h->pack_floats);
    place_encoder(p->ve, al(5 * RD), RD);
    p->vf = p->ve.att;
    p->wproj = al((int64_t)rows * D);
    p->partial = al(0);
    p->total = al.cur;
    if (p->total >= (int64_t(1) << 31)) { delete p; return fail("vsl_encode_windows: workspace of %lld floats exceeds the 2^31 offset range", (long long)p->total); }
    *out = p;
    return 0;
}

// vsl_encode_query: the operand packs and the query branch's own scratch of the inference plan -- the embedding concat E, the Embedding linear's
// output and ONE encoder application's y3, q, k, v, att on B Lq rows.  The output goes to the caller's buffer.  B = queries; the plan has no video
// side (T = 0 in its key).
int build_query_plan(vsl_handle_s* h, int Q, int Lq, int Lc, Plan** out) {
    const vsl_config& cf = h->cfg;
    if (Q < 1 || Lq < 1) return fail("vsl_encode_query: empty call (Q=%d queries, Lq=%d words)", Q, Lq);
    if (Lq > cf.max_pos_len)
        return fail("sequence length (Lq=%d) exceeds max_pos_len=%d: the positional table has no such row (layers_t7.py:196 -- IndexError in the reference)", Lq, cf.max_pos_len);
    if (Lq > MAX_LQ) return fail("Lq=%d > %d query words: the CQAttention kernels keep the whole query of a sample in LDS "
                                 "(the reference truncates at max_pos_len words, data_gen.py:188)", Lq, MAX_LQ);
    if ((int64_t)Q * Lq * D * 4 >= (int64_t(1) << 31))
        return fail("Q*Lq = %lld rows: an (R, 128) fp32 activation must stay below 2 GiB for the 32-bit buffer offsets of the conv-block kernels (encode the queries in chunks)", (long long)Q * Lq);
    if (Lc < 4 || Lc > MAX_LC) return fail("Lc=%d must be in [4, %d] (the widest char conv has kernel 4, layers_t7.py:52)", Lc, MAX_LC);
    Plan* p = new Plan();
    p->kind = PlanKind::EncodeQuery;
    p->B = Q; p->T = 0; p->Lq = Lq; p->Lc = Lc;
    const int64_t Rq = (int64_t)Q * Lq;
    p->qe.R = (int)Rq; p->qe.L = Lq;
    Bump al;
    p->pack = al(h->pack_floats);
    p->E = al(Rq * (cf.word_dim + 100)); p->qf = al(Rq * D);
    p->qe.y[3] = al(Rq * D); p->qe.q = al(Rq * D); p->qe.k = al(Rq * D); p->qe.v = al(Rq * D); p->qe.att = al(Rq * D);
    p->partial = al(0);
    p->total = al.cur;
    if (p->total >= (int64_t(1) << 31)) { delete p; return fail("encode-query workspace of %lld floats exceeds the 2^31 offset range", (long long)p->total); }
    *out = p;
    return 0;
}

int build_reduce_tables(vsl_handle_s* h, Plan* p, const std::vector<SlabRec>& recs);

// The training plan: every tensor the backward reads is saved, every backward temporary has its own buffer, and the partial arena behind them is
// laid out by a dry run of the backward.
// N > 0 (PlanKind::TrainShared): the video half -- VisualProjection's output, encoder application 0's saves and backward temporaries, dvf, and
// through the dry run its partial slabs -- is sized by N T rows, everything else by B; added: dCv (N, T, 128) and the grouping's CSR (N + 1 + B ints).
// The 2 GiB / 32-bit-offset limits apply to N T 128 and to B T 128 separately.
int build_train_plan(vsl_handle_s* h, int B, int T, int Lq, int Lc, Plan** out, int N = 0) {
    if (int rc = check_shape(h, B, T, Lq, Lc)) return rc;
    if (N > 0)
        if (int rc = check_video_shape(h, N, T, " (N = videos of the shared step)")) return rc;
    const vsl_config& cf = h->cfg;
    Plan* p = new Plan();
    p->B = B; p->T = T; p->Lq = Lq; p->Lc = Lc;
    if (N > 0) { p->N = N; p->kind = PlanKind::TrainShared; }
    const int64_t R = (int64_t)B * T, Rq = (int64_t)B * Lq, Rv = (int64_t)p->NV() * T;
    const int H = cf.num_heads, EW = cf.word_dim + 100;
    Bump al;
    p->pack = al(h->pack_floats);
    p->vf = al(Rv * D); p->E = al(Rq * EW); p->argpos = al((Rq * 100 + 3) / 4); p->qf = al(Rq * D);
    plan_encoder(al, p->ve, p->NV(), T, H); plan_encoder(al, p->qe, B, Lq, H);
    const bool rnn = cf.predictor == 0;
    if (rnn) {
        p->p1.R = p->p2.R = (int)R; p->p1.L = p->p2.L = T;
        for (int l = 0; l < 2; ++l) {
            LstmWs& w = p->lstm[l];
            w.gi = al(R * 4 * D); w.gates = al(R * 4 * D); w.cseq = al(R * D); w.tseq = al(R * D); w.hprev = al(R * D); w.out = al(R * D); w.dG = al(R * 4 * D);
            w.carry = al((int64_t)B * 2 * D);
        }
        p->p1.out = p->lstm[0].out; p->p2.out = p->lstm[1].out;
        if (rnn_fused_ok(B)) {
            p->h_gran = al(R * 2 * D); p->gi_gran = al(R * 8 * D); p->dg_gran = al(R * 8 * D); p->dx_gran = al(R * 2 * D);
            p->gran_floats = (p->dx_gran + R * 2 * D) - p->h_gran;      // the four allocations are consecutive
        }
    } else {
        plan_encoder(al, p->p1, B, T, H); plan_encoder(al, p->p2, B, T, H);
    }
    p->S = al(R * Lq); p->Srow = al(R * Lq); p->Scol = al(R * Lq); p->M = al(Rq * D); p->alpha = al(Rq);
    p->pooled = al((int64_t)B * D); p->pb = al((int64_t)B * D); p->cat = al(R * 4 * D);
    p->f1 = al(R * D); p->f2 = al(R * D); p->gated = al(R * D);
    p->hid_s = al(R * D); p->hid_e = al(R * D); p->lnf_s = al(R * D); p->lnf_e = al(R * D);
    p->loss_scratch = al(5 * (int64_t)B + 8);
    p->gz_s = al(R * D); p->gz_e = al(R * D); p->dfeat_s = al(R * D); p->dfeat_e = al(R * D);
    p->dxh_s = al(R * D); p->dxh_e = al(R * D); p->g_s1 = al(R * D); p->g_gated = al(R * D);
    for (int ap = 0; ap < (rnn ? 2 : 4); ++ap) {
        const int64_t Ra = ap == 1 ? Rq : ap == 0 ? Rv : R;
        EncTmp& t = p->tmp[ap];
        t.dr = al(Ra * D); t.dq = al(Ra * D * attn_dq_slabs(ap == 1 ? Lq : T)); t.dk = al(Ra * D); t.dv = al(Ra * D);
        t.go = al(Ra * D);
        for (int i = 0; i < 4; ++i) t.gz[i] = al(Ra * D);
        t.ga = al(Ra * D);
    }
    p->df2 = al(R * D); p->df1 = al(R * D); p->dC = al(R * D);
    {
        const int64_t nt = (T + TILE_M - 1) / TILE_M;
        p->cqP1 = al((int64_t)B * nt * 2 * Lq * D); p->cqP2 = al((int64_t)B * nt * Lq); p->cqP3 = al((int64_t)B * nt * Lq);
        p->cqP4 = al((int64_t)B * nt * Lq * D); p->cqP5 = al((int64_t)B * nt * D);
    }
    p->dSr = al(R * Lq); p->dSs = al(R * Lq); p->dQtot = al(Rq * D); p->dvf = al(Rv * D); p->dqf = al(Rq * D); p->dE = al(Rq * EW);
    if (N > 0) { p->dCv = al(Rv * D); p->csr = al(p->csr_members() + B); }
    p->partial = al(0);
    // dry-run the backward to lay out the partial arena and collect the reduction table
    std::vector<SlabRec> recs;
    Ctx c{h, p, nullptr, nullptr, true, nullptr};
    c.recs = &recs;
    run_backward(c);
    p->partial_floats = c.part_cur;
    al(p->partial_floats);
    p->total = al.cur;
    if (p->total >= (int64_t(1) << 31)) { delete p; return fail("workspace of %lld floats exceeds the 2^31 offset range of the reduction table", (long long)p->total); }
    if (int rc = build_reduce_tables(h, p, recs)) { free_plan(p); return rc; }
    *out = p;
    return 0;
}

// The device tables of the gradient reduction, from the partial slabs the dry run recorded.
// The reduction runs in two launches: `early` = parameters whose partials are complete before the final video/query fork
// (predictor, heads, CQ fusion), on a side stream; `late` = shared feature encoder, embedding stack, visual projection.
int build_reduce_tables(vsl_handle_s* h, Plan* p, const std::vector<SlabRec>& recs) {
    // group the records by destination (shared weights are written by up to 4 encoder applications)
    std::vector<ReduceSeg> segs;
    std::map<int, int> by_dst;
    for (const SlabRec& r : recs) {
        auto it = by_dst.find(r.dst);
        if (it == by_dst.end()) {
            ReduceSeg s;
            memset(&s, 0, sizeof s);
            s.dst = r.dst; s.n = r.n; s.rl = r.rl; s.ds = r.ds;
            by_dst[r.dst] = (int)segs.size();
            segs.push_back(s);
            it = by_dst.find(r.dst);
        }
        ReduceSeg& s = segs[it->second];
        if (s.n != r.n || s.nsrc >= 4) { return fail("internal: inconsistent partial slabs for param offset %d", r.dst); }
        s.src[s.nsrc] = (int)r.src; s.nslabs[s.nsrc] = r.nslabs; s.ss[s.nsrc] = r.ss; s.vn[s.nsrc] = r.vn;
        ++s.nsrc;
    }
    for (ReduceSeg& s : segs) {
        s.vec = (s.n % 4 == 0) && (s.rl % 4 == 0) && (s.ds % 4 == 0) && (s.dst % 4 == 0);
        for (int q = 0; q < s.nsrc; ++q) s.vec = s.vec && (s.src[q] % 4 == 0) && (s.ss[q] % 4 == 0) && (s.vn[q] % 4 == 0);
    }
    if (getenv("VSL_DEBUG_PLAN")) {
        int64_t tot = 0;
        for (const ReduceSeg& s : segs) {
            int64_t fl = 0; int ns = 0;
            for (int q = 0; q < s.nsrc; ++q) { fl += (int64_t)s.nslabs[q] * s.vn[q]; ns += s.nslabs[q]; }
            tot += fl;
            if (fl * 4 >= (256 << 10)) fprintf(stderr, "[plan] dst %8d n %7d nsrc %d slabs %5d  read %8.2f MiB\n", s.dst, s.n, s.nsrc, ns, fl * 4.0 / (1 << 20));
        }
        fprintf(stderr, "[plan] %zu segments, %.2f MiB of partial slabs read per step, partial arena %.2f MiB\n", segs.size(), tot * 4.0 / (1 << 20), p->partial_floats * 4.0 / (1 << 20));
    }
    // early / late split by destination: everything up to the end of the shared feature encoder's parameters is `late`
    // plus what k_cq_bwd_d produces on the query stream after the fork (w4Q, pooled-query weight, second half of / bias of
    // the CQConcatenate projection)
    const int late_end = h->P.w4C;       // params are laid out [embedding | visual | feature_encoder | cq... | predictor...]
    const int late_q[4] = {h->P.w4Q, h->P.pool_w, h->P.cat_b, h->P.cat_w + D};
    std::vector<int> blk;
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t i = 0; i < segs.size(); ++i) {
            bool late = segs[i].dst < late_end;
            for (int d : late_q) late = late || segs[i].dst == d;
            if (late != (pass == 1)) continue;
            for (int o = 0; o < segs[i].n; o += 256) { blk.push_back((int)i); blk.push_back(o); }
        }
        if (pass == 0) p->nblocks_early = (int)blk.size() / 2;
    }
    p->nblocks = (int)blk.size() / 2;
    HIP_OK(hipMalloc(&p->segs_dev, segs.size() * sizeof(ReduceSeg)));
    HIP_OK(hipMalloc(&p->blk2seg_dev, blk.size() * sizeof(int)));
    HIP_OK(hipMemcpy(p->segs_dev, segs.data(), segs.size() * sizeof(ReduceSeg), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(p->blk2seg_dev, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&p->sq_dev, (size_t)std::max(p->nblocks, 1) * sizeof(float)));
    {   // do the reduction blocks write every parameter gradient exactly once?  (then their sums of squares ARE the bucket's)
        std::vector<uint8_t> hit((size_t)h->param_floats, 0);
        bool once = true;
        for (const ReduceSeg& sg : segs)
            for (int i = 0; i < sg.n; ++i) {
                const int64_t d = (int64_t)sg.dst + (int64_t)(i / sg.rl) * sg.ds + (i % sg.rl);
                if (d < 0 || d >= h->param_floats || hit[(size_t)d]++) once = false;
            }
        for (const ParamInfo& pi : h->params)
            for (int64_t e = pi.off; e < pi.off + pi.numel; ++e) once = once && hit[(size_t)e] == 1;
        p->sq_cover = once;
    }
    return 0;
}

}  // namespace

void free_plan(Plan* p) {
    if (!p) return;
    if (p->segs_dev) (void)hipFree(p->segs_dev);
    if (p->blk2seg_dev) (void)hipFree(p->blk2seg_dev);
    if (p->sq_dev) (void)hipFree(p->sq_dev);
    delete p;
}

// Per-shape plans (workspace layout + reduction tables).  The collate narrows every batch to its own max T / Lq / Lc, so a
// long training run visits hundreds of shapes (Charades at batch 16: T in 40..128 x Lq in 4..10 x Lc in 5..12).  A plan is two small
// device tables (< 100 KB), a miss costs a rebuild, two hipMalloc and -- on eviction -- a device synchronise, so the cache holds every
// shape a realistic run sees (64 entries thrashed under shuffled real-data batches) and evicts the least recently used one
// beyond that.  (A forward and its backward use the same shape back to back, so a live plan is never evicted.)
constexpr size_t MAX_PLANS = 2048;
int get_plan(vsl_handle_s* h, int B, int T, int Lq, int Lc, Plan** out, PlanKind kind, int N) {
    if (kind == PlanKind::EncodeWindows) { }      // (N = the feature rows: part of the key, checked by the builder)
    else if (kind != PlanKind::TrainShared) N = 0;
    else if (N < 1) return fail("shared training step: N=%d videos (at least one)", N);
    auto key = std::make_tuple(B, T, Lq, Lc, N, kind);
    auto it = h->plans.find(key);
    if (it != h->plans.end()) { it->second->last_use = ++h->plan_clock; *out = it->second; return 0; }
    Plan* p = nullptr;
    int rc = 0;
    switch (kind) {
        case PlanKind::Train: rc = build_train_plan(h, B, T, Lq, Lc, &p); break;
        case PlanKind::TrainShared: rc = build_train_plan(h, B, T, Lq, Lc, &p, N); break;
        case PlanKind::Infer:
        case PlanKind::Localize:
        case PlanKind::LocalizePairs: rc = build_infer_plan(h, B, T, Lq, Lc, &p, kind); break;
        case PlanKind::Encode: rc = build_encode_plan(h, B, T, &p); break;
        case PlanKind::EncodeQuery: rc = build_query_plan(h, B, Lq, Lc, &p); break;
        case PlanKind::EncodeWindows: rc = build_windows_plan(h, B, T, N, &p); break;
    }
    if (rc) return rc;
    if (h->plans.size() >= MAX_PLANS) {
        auto victim = h->plans.begin();
        for (auto jt = h->plans.begin(); jt != h->plans.end(); ++jt)
            if (jt->second->last_use < victim->second->last_use) victim = jt;
        (void)hipDeviceSynchronize();            // its tables may still be read by an enqueued reduction
        if (h->sq_src == victim->second->sq_dev) { h->sq_src = nullptr; h->sq_grads = nullptr; }
        free_plan(victim->second);
        h->plans.erase(victim);
    }
    p->last_use = ++h->plan_clock;
    h->plans[key] = p;
    *out = p;
    return 0;
}

}  // namespace vsl
