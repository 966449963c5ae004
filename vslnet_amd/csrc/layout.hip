// The flat parameter layout (the reference's state_dict order), the weight-pack table derived from it, and the optimizer's per-element constants.
#include "host.hpp"

namespace vsl {

// ------------------------------------------------------------------------------------------------ parameters
struct ParamBuilder {
    vsl_handle_s* h;
    int add(const std::string& name, std::initializer_list<int64_t> dims) {
        ParamInfo p;
        p.name = name;
        p.ndim = (int)dims.size();
        p.numel = 1;
        int i = 0;
        for (auto d : dims) { p.dims[i++] = d; p.numel *= d; }
        p.off = h->param_floats;
        h->param_floats += (p.numel + 3) & ~int64_t(3);          // keep every tensor 16-byte aligned
        h->params.push_back(p);
        return (int)p.off;
    }
};

static void build_encoder_params(ParamBuilder& pb, const std::string& pre, EncP& e, int max_pos) {
    const int64_t d = D;
    e.pos = pb.add(pre + "pos_embedding.position_embeddings.weight", {max_pos, d});
    for (int i = 0; i < 4; ++i) {
        const std::string b = pre + "conv_block.depthwise_separable_conv." + std::to_string(i);
        e.dw[i] = pb.add(b + ".0.weight", {d, 1, 7});
        e.pw[i] = pb.add(b + ".1.weight", {d, d, 1});
        e.pwb[i] = pb.add(b + ".1.bias", {d});
    }
    for (int i = 0; i < 4; ++i) {
        const std::string b = pre + "conv_block.layer_norms." + std::to_string(i);
        e.lng[i] = pb.add(b + ".weight", {d});
        e.lnb[i] = pb.add(b + ".bias", {d});
    }
    const std::string a = pre + "attention_block.";
    e.qw = pb.add(a + "query.conv1d.weight", {d, d, 1});
    e.qb = pb.add(a + "query.conv1d.bias", {d});
    e.kw = pb.add(a + "key.conv1d.weight", {d, d, 1});
    e.kb = pb.add(a + "key.conv1d.bias", {d});
    e.vw = pb.add(a + "value.conv1d.weight", {d, d, 1});
    e.vb = pb.add(a + "value.conv1d.bias", {d});
    e.ln1g = pb.add(a + "layer_norm1.weight", {d});
    e.ln1b = pb.add(a + "layer_norm1.bias", {d});
    e.ln2g = pb.add(a + "layer_norm2.weight", {d});
    e.ln2b = pb.add(a + "layer_norm2.bias", {d});
    e.ow = pb.add(a + "out_layer.conv1d.weight", {d, d, 1});
    e.ob = pb.add(a + "out_layer.conv1d.bias", {d});
}

void build_params(vsl_handle_s* h) {
    // order == the reference's state_dict order restricted to trainable tensors
    const vsl_config& c = h->cfg;
    ParamBuilder pb{h};
    ModelP& P = h->P;
    const int64_t d = D;
    if (c.word_table) P.unk = pb.add("embedding_net.word_emb.word_emb.weight", {c.word_size, c.word_dim});      // rows 0 / 1 stand where pad_vec / unk_vec do
    else P.unk = pb.add("embedding_net.word_emb.unk_vec", {1, c.word_dim});
    P.char_tab = pb.add("embedding_net.char_emb.char_emb.weight", {c.char_size, c.char_dim});
    const int ch[4] = {10, 20, 30, 40};
    for (int i = 0; i < 4; ++i) {
        const std::string b = "embedding_net.char_emb.char_convs." + std::to_string(i) + ".0";
        P.ccw[i] = pb.add(b + ".weight", {ch[i], c.char_dim, 1, i + 1});
        P.ccb[i] = pb.add(b + ".bias", {ch[i]});
    }
    P.emb_w = pb.add("embedding_net.linear.conv1d.weight", {d, c.word_dim + 100, 1});
    P.emb_b = pb.add("embedding_net.linear.conv1d.bias", {d});
    P.va_w = pb.add("video_affine.linear.conv1d.weight", {d, c.video_feature_dim, 1});
    P.va_b = pb.add("video_affine.linear.conv1d.bias", {d});
    build_encoder_params(pb, "feature_encoder.", P.fe, c.max_pos_len);
    P.w4C = pb.add("cq_attention.w4C", {d, 1});
    P.w4Q = pb.add("cq_attention.w4Q", {d, 1});
    P.w4mlu = pb.add("cq_attention.w4mlu", {1, 1, d});
    P.cqa_w = pb.add("cq_attention.cqa_linear.conv1d.weight", {d, 4 * d, 1});
    P.cqa_b = pb.add("cq_attention.cqa_linear.conv1d.bias", {d});
    P.pool_w = pb.add("cq_concat.weighted_pool.weight", {d, 1});
    P.cat_w = pb.add("cq_concat.conv1d.conv1d.weight", {d, 2 * d, 1});
    P.cat_b = pb.add("cq_concat.conv1d.conv1d.bias", {d});
    P.hl_w = pb.add("highlight_layer.conv1d.conv1d.weight", {1, d, 1});
    P.hl_b = pb.add("highlight_layer.conv1d.conv1d.bias", {1});
    if (c.predictor == 0) {          // rnn head (layers_t7.py:319-321): two nn.LSTM(d, d), gate order i,f,g,o
        const char* nm[2] = {"predictor.start_encoder.lstm.", "predictor.end_encoder.lstm."};
        for (int l = 0; l < 2; ++l) {
            const std::string a = nm[l];
            P.l_wih[l] = pb.add(a + "weight_ih_l0", {4 * d, d});
            P.l_whh[l] = pb.add(a + "weight_hh_l0", {4 * d, d});
            P.l_bih[l] = pb.add(a + "bias_ih_l0", {4 * d});
            P.l_bhh[l] = pb.add(a + "bias_hh_l0", {4 * d});
        }
        P.sln_g = P.sln_b = P.eln_g = P.eln_b = -1;
    } else {
        build_encoder_params(pb, "predictor.encoder.", P.pe, c.max_pos_len);
        P.sln_g = pb.add("predictor.start_layer_norm.weight", {d});
        P.sln_b = pb.add("predictor.start_layer_norm.bias", {d});
        P.eln_g = pb.add("predictor.end_layer_norm.weight", {d});
        P.eln_b = pb.add("predictor.end_layer_norm.bias", {d});
    }
    P.s0w = pb.add("predictor.start_block.0.conv1d.weight", {d, 2 * d, 1});
    P.s0b = pb.add("predictor.start_block.0.conv1d.bias", {d});
    P.s1w = pb.add("predictor.start_block.2.conv1d.weight", {1, d, 1});
    P.s1b = pb.add("predictor.start_block.2.conv1d.bias", {1});
    P.e0w = pb.add("predictor.end_block.0.conv1d.weight", {d, 2 * d, 1});
    P.e0b = pb.add("predictor.end_block.0.conv1d.bias", {d});
    P.e1w = pb.add("predictor.end_block.2.conv1d.weight", {1, d, 1});
    P.e1b = pb.add("predictor.end_block.2.conv1d.bias", {1});
}

// ------------------------------------------------------------------------------------------------ weight packs
struct PackBuilder {
    vsl_handle_s* h;
    // forward pack of W (N x K, leading dim ld): Bm[k][c] = W[c][k]
    int fwd(int src, int N, int Kd, int ld) {
        const int dst = (int)h->pack_floats;
        h->pack_floats += (int64_t)pack_size(Kd, N);
        h->jobs.push_back(PackJob{src, dst, Kd, N, ld, 0, N, 0, 0});
        return dst;
    }
    // split packs (three bf16 planes, common.hpp pack3_index) of the same two operands
    // (kpad: the contraction extent is zero-padded to a multiple of it -- a K-chunked kernel then needs no tail guards)
    int fwd3(int src, int N, int Kd, int ld, int kpad = 16) {
        const int dst = (int)h->pack_floats, Kp = (Kd + kpad - 1) / kpad * kpad;
        h->pack_floats += (int64_t)((pack3_floats(Kp, N) + 3) & ~size_t(3));
        h->jobs.push_back(PackJob{src, dst, Kd, N, ld, 6, N, 0, 0, Kp, Kp});
        return dst;
    }
    int tr3(int src, int N, int Kd, int ld, int kpad = 16) {
        const int dst = (int)h->pack_floats, Np = (N + kpad - 1) / kpad * kpad;
        h->pack_floats += (int64_t)((pack3_floats(Np, Kd) + 3) & ~size_t(3));
        h->jobs.push_back(PackJob{src, dst, N, Kd, ld, 7, Kd, 0, 0, Np, Np});
        return dst;
    }
    // transpose pack of W (N x K): Bm[k = n][c] = W[n][c], ncols = K
    int tr(int src, int N, int Kd, int ld) {
        const int dst = (int)h->pack_floats;
        h->pack_floats += (int64_t)pack_size(N, Kd);
        h->jobs.push_back(PackJob{src, dst, N, Kd, ld, 1, Kd, 0, 0});
        return dst;
    }
};
static void build_encoder_packs(PackBuilder& pk, vsl_handle_s* h, const EncP& e, EncPk& k) {
    for (int i = 0; i < 4; ++i) { k.pw_f[i] = pk.fwd(e.pw[i], D, D, D); k.pw_t[i] = pk.tr(e.pw[i], D, D, D); }
    // fused QKV operand: forward pack has 384 columns [q | k | v]; transpose pack has 384 contraction rows
    k.qkv_f = (int)h->pack_floats;
    h->pack_floats += (int64_t)pack_size(D, 3 * D);
    const int qkv[3] = {e.qw, e.kw, e.vw};
    for (int i = 0; i < 3; ++i) h->jobs.push_back(PackJob{qkv[i], k.qkv_f, D, D, D, 0, 3 * D, 0, i * D});
    k.qkv_t = (int)h->pack_floats;
    h->pack_floats += (int64_t)pack_size(3 * D, D);
    for (int i = 0; i < 3; ++i) h->jobs.push_back(PackJob{qkv[i], k.qkv_t, D, D, D, 1, D, i * D, 0});
    k.o_f = pk.fwd(e.ow, D, D, D);
    k.o_t = pk.tr(e.ow, D, D, D);
    // split packs (fp32 grade on the bf16 matrix cores)
    for (int i = 0; i < 4; ++i) { k.pw_f3[i] = pk.fwd3(e.pw[i], D, D, D); k.pw_t3[i] = pk.tr3(e.pw[i], D, D, D); }
    k.qkv_f3 = (int)h->pack_floats;
    h->pack_floats += (int64_t)((pack3_floats(D, 3 * D) + 3) & ~size_t(3));
    for (int i = 0; i < 3; ++i) h->jobs.push_back(PackJob{qkv[i], k.qkv_f3, D, D, D, 6, 3 * D, 0, i * D, D, D});
    k.qkv_t3 = (int)h->pack_floats;
    h->pack_floats += (int64_t)((pack3_floats(3 * D, D) + 3) & ~size_t(3));
    for (int i = 0; i < 3; ++i) h->jobs.push_back(PackJob{qkv[i], k.qkv_t3, D, D, D, 7, D, i * D, 0, 3 * D, D});
    k.o_f3 = pk.fwd3(e.ow, D, D, D);
    k.o_t3 = pk.tr3(e.ow, D, D, D);
}
void build_packs(vsl_handle_s* h) {
    const vsl_config& c = h->cfg;
    PackBuilder pk{h};
    ModelPk& K = h->K;
    const ModelP& P = h->P;
    K.va_f = pk.fwd(P.va_w, D, c.video_feature_dim, c.video_feature_dim);
    // bf16 throughput mode: the same weight rounded to bfloat16 in the operand layout of v_mfma_f32_32x32x16_bf16
    K.va_f16 = (int)h->pack_floats;
    h->pack_floats += (int64_t)((c.video_feature_dim + 15) / 16) * D * 16 / 2;
    h->jobs.push_back(PackJob{P.va_w, K.va_f16, c.video_feature_dim, D, c.video_feature_dim, 5, D, 0, 0});
    K.va_f3 = pk.fwd3(P.va_w, D, c.video_feature_dim, c.video_feature_dim, 128);      // split pack: fp32 grade on the bf16 matrix cores
    K.emb_f = pk.fwd(P.emb_w, D, c.word_dim + 100, c.word_dim + 100);
    K.emb_t = pk.tr(P.emb_w, D, c.word_dim + 100, c.word_dim + 100);
    K.emb_f3 = pk.fwd3(P.emb_w, D, c.word_dim + 100, c.word_dim + 100);
    {   // data-gradient operand with its column count padded to whole 128-column tiles (the pad columns are never stored)
        const int EWc = (c.word_dim + 100 + 127) / 128 * 128;
        K.emb_t3_cols = EWc;
        K.emb_t3 = (int)h->pack_floats;
        h->pack_floats += (int64_t)((pack3_floats(D, EWc) + 3) & ~size_t(3));
        h->jobs.push_back(PackJob{P.emb_w, K.emb_t3, D, c.word_dim + 100, c.word_dim + 100, 7, EWc, 0, 0, D, D});
    }
    build_encoder_packs(pk, h, P.fe, K.fe);
    if (c.predictor == 0) {
        for (int l = 0; l < 2; ++l) {
            K.l_f3[l] = pk.fwd3(P.l_wih[l], 4 * D, D, D);    // gi = x W_ih^T  : (R,128) x (128,512), split pack
            K.l_t[l] = pk.tr(P.l_wih[l], 4 * D, D, D);       // dx = dG W_ih   : (R,512) x (512,128)
            K.l_t3[l] = pk.tr3(P.l_wih[l], 4 * D, D, D, 128);
            for (int bw = 0; bw < 2; ++bw) {                 // W_hh in the register order of k_lstm1_fwd / k_lstm1_bwd
                (bw ? K.l_hb : K.l_hf)[l] = (int)h->pack_floats;
                h->jobs.push_back(PackJob{P.l_whh[l], (int)h->pack_floats, LSTM_IMG_FLOATS, 1, 0, 9 + bw, 1, 0, 0});
                h->pack_floats += LSTM_IMG_FLOATS;
            }
            if (l == 1) for (int bw = 0; bw < 2; ++bw) {     // the end LSTM's W_ih likewise: the projection workgroups of k_rnn_fwd / k_rnn_bwd
                (bw ? K.l_ib : K.l_if) = (int)h->pack_floats;
                h->jobs.push_back(PackJob{P.l_wih[1], (int)h->pack_floats, LSTM_IMG_FLOATS, 1, 0, 9 + bw, 1, 0, 0});
                h->pack_floats += LSTM_IMG_FLOATS;
            }
        }
        K.zero128 = (int)h->pack_floats;                    // a zero bias vector for the bias-less GEMM above
        h->pack_floats += D;
        h->jobs.push_back(PackJob{0, K.zero128, D, 1, 0, 4, 1, 0, 0});
    } else {
        build_encoder_packs(pk, h, P.pe, K.pe);
    }
    K.cqa_f = pk.fwd(P.cqa_w, D, 4 * D, 4 * D);
    K.cqa_t = pk.tr(P.cqa_w, D, 4 * D, 4 * D);
    K.cat1_f = pk.fwd(P.cat_w, D, D, 2 * D);          // first half of the (128, 256) CQConcatenate weight
    K.cat1_t = pk.tr(P.cat_w, D, D, 2 * D);
    K.s0_f = pk.fwd(P.s0w, D, 2 * D, 2 * D);
    K.s0_t = pk.tr(P.s0w, D, 2 * D, 2 * D);
    K.e0_f = pk.fwd(P.e0w, D, 2 * D, 2 * D);
    K.e0_t = pk.tr(P.e0w, D, 2 * D, 2 * D);
    // char-conv weights as one [ci][4 taps][100 channels] image; each job writes all 4 tap slots of its channels (zero
    // beyond the kernel width), so the image is fully defined every step
    K.ccw_img = (int)h->pack_floats;
    h->pack_floats += (int64_t)c.char_dim * 400;
    const int chn[4] = {10, 20, 30, 40};
    int oc0 = 0;
    for (int i = 0; i < 4; ++i) {
        PackJob j{P.ccw[i], K.ccw_img, chn[i] * c.char_dim * 4, 1, i + 1, 3, c.char_dim, 0, oc0};
        h->jobs.push_back(j);
        oc0 += chn[i];
    }
    // the same weights as the B operands of the embedding backward's dCe product, in lane order (kernels_params.hip k_pack, type 8)
    K.ccw_imgb = (int)h->pack_floats;
    const int ebn = ((c.char_dim + 15) / 16) * EB_IMG_Q * 64;
    h->pack_floats += ebn;
    oc0 = 0;
    for (int i = 0; i < 4; ++i) {
        PackJob j{P.ccw[i], K.ccw_imgb, ebn, 1, i + 1, 8, c.char_dim, chn[i], oc0};
        h->jobs.push_back(j);
        oc0 += chn[i];
    }
}

// The pack table as the forwards launch it: jobs nobody reads dropped, the rest ordered by the launch they belong to
// (vsl_handle_s::jobs_char / jobs_first / jobs_va / jobs_query).
void finish_pack_jobs(vsl_handle_s* h) {
    const vsl_config& cfg = h->cfg;
    const ModelPk& K = h->K;
    {
        // Drop the pack jobs whose operand no kernel reads: the fp32 packs of the GEMMs that run as split products and the split packs of the
        // attention output projection (it stays on the fp32-input MFMA).
        // The regions stay in the pack buffer (offsets are fixed); k_pack just does a third less work every step.
        std::vector<int> dead;
        auto enc = [&](const EncPk& e) {
            if (&e != &K.fe) { dead.push_back(e.o_f3); dead.push_back(e.o_t3); }      // (the feature encoder's: read by the sample-local query kernels, kernels_query.hip)
            for (int i = 0; i < 4; ++i) { dead.push_back(e.pw_f[i]); dead.push_back(e.pw_t[i]); }
            dead.push_back(e.qkv_f); dead.push_back(e.qkv_t);
        };
        enc(K.fe);
        if (cfg.predictor != 0) enc(K.pe);
        dead.push_back(K.va_f); dead.push_back(K.emb_t);
        if ((cfg.word_dim + 100) % 16 == 0) dead.push_back(K.emb_f);
        if (cfg.predictor == 0) for (int l = 0; l < 2; ++l) dead.push_back(K.l_t[l]);        // the rnn head's dx GEMM reads the split pack l_t3
        h->jobs.erase(std::remove_if(h->jobs.begin(), h->jobs.end(), [&](const PackJob& j) {
                          return std::find(dead.begin(), dead.end(), j.dst) != dead.end(); }), h->jobs.end());
    }
    {   // Three pack launches per forward (forward_full): what VisualProjection and the shared feature encoder's forward read goes first on the
        // main stream, the embedding stack's operands on the query stream, everything else (CQ fusion, heads, predictor encoder, every
        // data-gradient pack) on the weight-gradient stream, which is idle in the forward -- the step no longer opens with ONE 11 us launch
        // that packs 2.7 MB before its first kernel may start.
        auto in = [](int dst, std::initializer_list<int> set) { return std::find(set.begin(), set.end(), dst) != set.end(); };
        auto cls = [&](const PackJob& j) {
            const EncPk& f = K.fe;
            if (j.dst == K.ccw_img) return 0;
            if (in(j.dst, {f.pw_f[0], f.pw_f[1], f.pw_f[2], f.pw_f[3], f.qkv_f, f.o_f, f.pw_f3[0], f.pw_f3[1], f.pw_f3[2], f.pw_f3[3], f.qkv_f3, f.o_f3})) return 1;
            if (in(j.dst, {K.va_f, K.va_f16, K.va_f3})) return 2;      // (last of the first launch: vsl_localize leaves these out, vsl_encode_video packs 1 and 2)
            if (in(j.dst, {K.emb_f, K.emb_f3})) return 3;
            return 4;
        };
        std::stable_sort(h->jobs.begin(), h->jobs.end(), [&](const PackJob& a, const PackJob& b) { return cls(a) < cls(b); });
        for (const PackJob& j : h->jobs) {
            const int k = cls(j);
            h->jobs_char += k == 0; h->jobs_first += k == 1 || k == 2; h->jobs_va += k == 2; h->jobs_query += k == 3;
        }
    }
}

// the optimizer's device-side constants (first use): decay flags, scratch of the two-kernel step
int ensure_opt_state(vsl_handle_s* h) {
    if (h->decay_dev) return 0;
    std::vector<uint8_t> mask((size_t)h->param_floats, 0);          // VSLNet_t7.py:9-13: no decay for bias / layer_norm / LayerNorm parameters
    for (const ParamInfo& p : h->params) {
        const bool nd = p.name.find("bias") != std::string::npos || p.name.find("layer_norm") != std::string::npos ||
                        p.name.find("LayerNorm") != std::string::npos;
        if (!nd) std::fill(mask.begin() + p.off, mask.begin() + p.off + p.numel, (uint8_t)1);
    }
    if (hipMalloc(&h->decay_dev, mask.size()) != hipSuccess || hipMalloc(&h->opt_scratch, (OPT_BLOCKS + 4) * sizeof(float)) != hipSuccess)
        return fail("optimizer state: hipMalloc failed");
    if (hipMemcpy(h->decay_dev, mask.data(), mask.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail("optimizer state: hipMemcpy failed");
    return 0;
}

}  // namespace vsl
