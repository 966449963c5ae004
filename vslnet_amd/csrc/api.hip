// C ABI of libvslnet_hip.so (declared in include/vslnet_hip.h).  Every entry point checks its arguments and states its own refusals; the ones
// that enqueue a launch sequence (vsl_forward, vsl_forward_shared, vsl_encode_video, vsl_localize, vsl_encode_query, vsl_localize_pairs, vsl_highlight_pairs, vsl_encode_windows, the backward's three entry points, vsl_input_grads) then go
// through ONE path, enqueue(): plan of the shape, the call's context, the CallScope, the sequence of forward.hip / backward.hip, the launch-error
// check and, for a forward, record_forward(): what it left for the calls behind it.  (layout.hip, plan.hip do the rest; the vsl_profile_* entry
// points live with the profiler in streams.hip.)  Host code only -- no device code lives here.
#include "host.hpp"

using namespace vsl;

// the bf16 throughput mode reads the features eight to a lane
static int check_bf16_features(const vsl_handle_s* h, const void* video_features_bf16) {
    if (video_features_bf16 && (h->cfg.video_feature_dim % 8 != 0))
        return fail("bf16 features need video_feature_dim %% 8 == 0 (got %d)", h->cfg.video_feature_dim);
    return 0;
}

static int check_io(vsl_handle_s* h, const vsl_io* io) {
    if (!h || !io) return fail("null handle / io");
    if (!io->params || (!h->cfg.word_table && (!io->pad_vec || !io->glove_vec)) || !io->word_ids || !io->char_ids || (!io->video_features && !io->video_features_bf16) ||
        !io->v_mask || !io->q_mask || !io->h_score || !io->start_logits || !io->end_logits || !io->workspace)
        return fail("vsl_io has a null device pointer");
    return check_bf16_features(h, io->video_features_bf16);
}

// The vsl_io of an evaluation-only entry point (vsl_encode_video, vsl_localize, ...): zeroed but for the shape of its plan's key, the parameters, the
// workspace and inference = 1; the entry point adds the pointers its sequence reads.
static vsl_io eval_io(int B, int T, int Lq, int Lc, const float* params, float* workspace) {
    vsl_io io;
    memset(&io, 0, sizeof io);
    io.B = B; io.T = T; io.Lq = Lq; io.Lc = Lc;
    io.params = params; io.workspace = workspace; io.inference = 1;
    return io;
}

static int workspace_floats(vsl_handle_s* h, PlanKind kind, int B, int T, int Lq, int Lc, int64_t* out, int N = 0) {
    if (!h || !out) return fail("null argument");
    Plan* p = nullptr;
    if (int rc = get_plan(h, B, T, Lq, Lc, &p, kind, N)) return rc;
    *out = p->total;
    return 0;
}

// A forward has been enqueued: what the calls behind it find.  infer_ws = the workspace of the last forward that saved nothing, cleared only by a
// saved-path forward in that same workspace.
static void record_forward(vsl_handle_s* h, vsl_handle_s::LastFwd kind, const float* workspace, int shared_N) {
    h->last_fwd = kind;
    h->bwd_ws = nullptr; h->bwd_stepped = false;
    if (kind == vsl_handle_s::FwdShared) h->shared_N = shared_N;
    if (kind == vsl_handle_s::FwdInfer) h->infer_ws = workspace;
    else if (h->infer_ws == workspace) h->infer_ws = nullptr;
}

// One enqueuing call: the plan of the io's shape, the call's context, the call's bookkeeping, `seq` (which enqueues), the launch-error check, and
// -- `fwd` other than FwdNone: the call is a forward of that kind -- the record of it.  `rows`: the feature rows in the key of an EncodeWindows plan.
template <class Seq>
static int enqueue(vsl_handle_s* h, const vsl_io* io, PlanKind kind, const vsl_shared_io* sh, void* hip_stream, vsl_handle_s::LastFwd fwd, Seq&& seq, int rows = 0) {
    Plan* p = nullptr;
    if (int rc = get_plan(h, io->B, io->T, io->Lq, io->Lc, &p, kind, sh ? sh->N : rows)) return rc;
    Ctx c{h, p, io, (hipStream_t)hip_stream, false, io->workspace};
    c.main = c.s;
    c.sh = sh;
    CallScope scope(h);
    seq(c);
    HIP_OK(hipGetLastError());
    if (fwd != vsl_handle_s::FwdNone) record_forward(h, fwd, io->workspace, sh ? sh->N : 0);
    return 0;
}

// vsl_workspace_offset / vsl_shared_workspace_offset behind a forward that saved nothing: refused (-2)
static bool saved_nothing(vsl_handle_s* h, const char* who) {
    if (!h || h->last_fwd != vsl_handle_s::FwdInfer) return false;
    fail("%s: the last forward saved nothing (inference mode): there is no saved activation to point at", who);
    return true;
}

static int64_t plan_offset(vsl_handle_s* h, const Plan* p, const char* name);

extern "C" {

const char* vsl_last_error(void) { return g_err.c_str(); }

int vsl_create(const vsl_config* cfg, vsl_handle* out) {
    if (!cfg || !out) return fail("null argument");
    if (cfg->dim != D) return fail("configs.dim=%d: the HIP kernels are specialised for dim=128", cfg->dim);
    if (cfg->num_heads <= 0 || cfg->dim % cfg->num_heads != 0)
        return fail("The channels (%d) is not a multiple of attention heads (%d)", cfg->dim, cfg->num_heads);   // layers_t7.py:146
    if (!attn_heads_supported(cfg->num_heads))
        return fail("num_heads=%d: the attention kernels support num_heads 1, 2, 4, 8 and 16 (head sizes 128, 64, 32, 16 and 8)", cfg->num_heads);
    if (cfg->predictor != 0 && cfg->predictor != 1) return fail("predictor must be 0 ('rnn') or 1 ('transformer'), got %d", cfg->predictor);
    if (cfg->video_feature_dim <= 0 || cfg->video_feature_dim % 4) return fail("video_feature_dim=%d must be a positive multiple of 4 (rows are read as float4)", cfg->video_feature_dim);
    if ((cfg->word_dim + 100) % 8) return fail("word_dim + 100 = %d must be a multiple of 8", cfg->word_dim + 100);
    if (cfg->word_table != 0 && cfg->word_table != 1) return fail("word_table must be 0 (frozen vectors + unk_vec) or 1 (trainable table), got %d", cfg->word_table);
    if (cfg->word_table && (cfg->word_dim > 512 || cfg->word_size < 2)) return fail("trainable word table: word_dim=%d must be <= 512 and word_size=%d >= 2", cfg->word_dim, cfg->word_size);
    if (cfg->char_dim <= 0 || cfg->char_dim > 128) return fail("char_dim=%d must be in [1, 128]", cfg->char_dim);
    if (cfg->char_size <= 0 || cfg->char_size * cfg->char_dim > 65536) return fail("char table of %d x %d floats: every embedding-backward workgroup writes one partial copy, 65536 floats is the limit", cfg->char_size, cfg->char_dim);
    if (cfg->max_pos_len <= 0 || cfg->word_size < 2) return fail("bad max_pos_len / word_size");
    if (cfg->drop_rate < 0.f || cfg->drop_rate >= 1.f) return fail("drop_rate must be in [0, 1)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device available: libvslnet_hip needs an MI355X (gfx950)");
    vsl_handle_s* h = new vsl_handle_s();
    h->cfg = *cfg;
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) h->cus = 0;
    }
    build_params(h);
    build_packs(h);
    finish_pack_jobs(h);
    if (hipMalloc(&h->loss_counter, sizeof(unsigned)) != hipSuccess || hipMemset(h->loss_counter, 0, sizeof(unsigned)) != hipSuccess) {
        delete h;
        return fail("hipMalloc of the loss counter failed");
    }
    if (hipMalloc(&h->jobs_dev, h->jobs.size() * sizeof(PackJob)) != hipSuccess ||
        hipMemcpy(h->jobs_dev, h->jobs.data(), h->jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice) != hipSuccess) {
        delete h;
        return fail("hipMalloc/hipMemcpy of the pack table failed");
    }
    {
        h->multi_stream = switch_on("VSL_MULTI_STREAM", true);     // (per handle: read at every vsl_create)
        if (h->multi_stream)
            for (int k = 0; k < 2; ++k) {
                // side(1) carries the weight gradients: nothing waits for them until the final reduction, so it runs at the
                // lowest priority the device offers and leaves CUs to the dependent chain
                int lo = 0, hi = 0;
                (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
                const int prio = k == 1 ? lo : 0;       // (the query stream's priority makes no difference either way: profiles/r03_notes.md)
                if (hipStreamCreateWithPriority(&h->side[k], hipStreamNonBlocking, prio) != hipSuccess) { h->side[k] = nullptr; (void)hipGetLastError(); }
            }
    }
    *out = h;
    return 0;
}

int vsl_destroy(vsl_handle h) {
    if (!h) return 0;
    for (int k = 0; k < 2; ++k) if (h->side[k]) (void)hipStreamDestroy(h->side[k]);
    for (hipEvent_t e : h->sync_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->stop_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->prof_pool) (void)hipEventDestroy(e);
    for (auto& kv : h->plans) free_plan(kv.second);
    if (h->jobs_dev) (void)hipFree(h->jobs_dev);
    if (h->loss_counter) (void)hipFree(h->loss_counter);
    if (h->decay_dev) (void)hipFree(h->decay_dev);
    if (h->opt_scratch) (void)hipFree(h->opt_scratch);
    delete h;
    return 0;
}

int vsl_param_count(vsl_handle h) { return h ? (int)h->params.size() : 0; }
int64_t vsl_param_floats(vsl_handle h) { return h ? h->param_floats : 0; }
int vsl_param_info(vsl_handle h, int index, char* name, int name_cap, int64_t* offset, int64_t* numel, int32_t* ndim,
                   int64_t dims[4]) {
    if (!h || index < 0 || index >= (int)h->params.size()) return fail("bad parameter index");
    const ParamInfo& p = h->params[index];
    if (name && name_cap > 0) { strncpy(name, p.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (offset) *offset = p.off;
    if (numel) *numel = p.numel;
    if (ndim) *ndim = p.ndim;
    if (dims) for (int i = 0; i < 4; ++i) dims[i] = i < p.ndim ? p.dims[i] : 1;
    return 0;
}

int vsl_workspace_floats(vsl_handle h, int B, int T, int Lq, int Lc, int64_t* out) { return workspace_floats(h, PlanKind::Train, B, T, Lq, Lc, out); }

int vsl_inference_workspace_floats(vsl_handle h, int B, int T, int Lq, int Lc, int64_t* out) { return workspace_floats(h, PlanKind::Infer, B, T, Lq, Lc, out); }

int64_t vsl_workspace_offset(vsl_handle h, int B, int T, int Lq, int Lc, const char* name) {
    Plan* p = nullptr;
    if (saved_nothing(h, "vsl_workspace_offset")) return -2;
    if (!h || !name || get_plan(h, B, T, Lq, Lc, &p)) return -1;
    return plan_offset(h, p, name);
}

int64_t vsl_shared_workspace_offset(vsl_handle h, int B, int N, int T, int Lq, int Lc, const char* name) {
    Plan* p = nullptr;
    if (saved_nothing(h, "vsl_shared_workspace_offset")) return -2;
    if (!h || !name || get_plan(h, B, T, Lq, Lc, &p, PlanKind::TrainShared, N)) return -1;
    const std::string n = name;
    if (n == "d_venc_video") return p->dCv;
    if (n == "group_start") return p->csr;
    if (n == "group_members") return p->csr + p->csr_members();
    return plan_offset(h, p, name);
}

}  // extern "C"

static int64_t plan_offset(vsl_handle_s* h, const Plan* p, const char* name) {
    const std::string n = name;
    const std::pair<const char*, int64_t> tab[] = {
        {"video_affine", p->vf}, {"embedding_net", p->qf}, {"emb_concat", p->E}, {"venc", p->ve.out}, {"qenc", p->qe.out},
        {"venc_x0", p->ve.x0}, {"venc_conv0", p->ve.y[0]}, {"venc_conv3", p->ve.y[3]}, {"venc_q", p->ve.q}, {"venc_k", p->ve.k},
        {"venc_v", p->ve.v}, {"venc_att", p->ve.att}, {"venc_r", p->ve.r}, {"qenc_conv3", p->qe.y[3]}, {"qenc_att", p->qe.att},
        {"cq_score", p->S}, {"cq_srow", p->Srow}, {"cq_scol", p->Scol}, {"cq_M", p->M}, {"cq_attention", p->f1},
        {"cq_concat", p->f2}, {"gated", p->gated}, {"pred_s", p->p1.out}, {"pred_e", p->p2.out},
        {"d_gated_enc", p->g_gated}, {"d_gated_hs", p->dxh_s}, {"d_gated_he", p->dxh_e}, {"d_venc", p->dC}, {"d_qenc", p->dQtot}, {"d_video_affine", p->dvf}, {"d_embedding_net", p->dqf},
        {"d_pred_s", p->g_s1}, {"d_pred_s_head", p->dfeat_s}, {"d_cq_concat", p->df2}, {"d_cq_attention", p->df1}, {"d_emb_concat", p->dE}};
    for (auto& kv : tab) if (n == kv.first) return kv.second;
    // ReLU decisions of the forward (parity tests count sign flips against the oracle): "relu_<enc>_<layer>" = (R, 4) uint32
    // bit-masks of conv layer 0..3 of venc / qenc / p1 / p2 ; "hid_s" / "hid_e" = post-ReLU activations of the span heads
    if (n == "hid_s") return p->hid_s;
    if (n == "hid_e") return p->hid_e;
    const std::pair<const char*, const EncWs*> encs[] = {{"relu_venc_", &p->ve}, {"relu_qenc_", &p->qe}, {"relu_p1_", &p->p1}, {"relu_p2_", &p->p2}};
    // "<enc>_y<layer>": output of conv layer 0..3 of that pass (R, 128) ; "<enc>_x0": its input + positional rows
    const std::pair<const char*, const EncWs*> acts[] = {{"venc_y", &p->ve}, {"qenc_y", &p->qe}, {"p1_y", &p->p1}, {"p2_y", &p->p2}};
    for (auto& kv : acts) {
        const size_t len = strlen(kv.first);
        if (h->cfg.predictor == 0 && (kv.second == &p->p1 || kv.second == &p->p2)) continue;
        if (n.size() == len + 1 && n.compare(0, len, kv.first) == 0 && n[len] >= '0' && n[len] <= '3') return kv.second->y[n[len] - '0'];
        if (n.size() == len + 1 && n.compare(0, len - 1, kv.first, len - 1) == 0 && n.compare(len - 1, 2, "x0") == 0) return kv.second->x0;
    }
    for (auto& kv : encs) {
        const size_t len = strlen(kv.first);
        if (n.size() == len + 1 && n.compare(0, len, kv.first) == 0 && n[len] >= '0' && n[len] <= '3') {
            if (h->cfg.predictor == 0 && (kv.second == &p->p1 || kv.second == &p->p2)) return -1;
            return kv.second->mask[n[len] - '0'];
        }
    }
    return -1;
}

// the checks vsl_backward and vsl_backward_shared share: the seeds or the fused loss, the gradient bucket, the fused optimizer step
static int check_backward_io(vsl_handle_s* h, const vsl_io* io, const char* who) {
    if (const vsl_loss_io* l = io->fused_loss) {
        if (!l->start_labels || !l->end_labels || !l->h_labels || !l->losses) return fail("%s: fused_loss has a null pointer", who);
        if (!l->d_start_logits || !l->d_end_logits || !l->d_h_score) return fail("%s: fused_loss needs the three gradient seed outputs", who);
        if (!io->grads) return fail("%s needs grads", who);
    } else
    if (!io->d_start_logits || !io->d_end_logits || !io->grads) return fail("%s needs d_start_logits, d_end_logits and grads", who);
    if (const vsl_fused_step* fs = io->fused_step) {
        if (!fs->params || !fs->exp_avg || !fs->exp_avg_sq) return fail("%s: fused_step needs params, exp_avg and exp_avg_sq", who);
        if (fs->hp.step < 1) return fail("%s: fused_step.hp.step must be >= 1 (got %d)", who, fs->hp.step);
        if (io->early_grads_event) return fail("%s: fused_step (single process) and early_grads_event (data parallel) exclude each other", who);
        if (int rc = ensure_opt_state(h)) return rc;
    }
    return 0;
}

static int check_shared_io(const vsl_io* io, const vsl_shared_io* sh, const char* who) {
    if (!sh) return fail("%s: the vsl_shared_io is NULL", who);
    if (sh->N < 1) return fail("%s: N=%d videos (at least one)", who, sh->N);
    if (!sh->video_index) return fail("%s: video_index is NULL (the video of each query)", who);
    if (!sh->video_v_mask) return fail("%s: video_v_mask is NULL (the (N, T) clip mask of the videos)", who);
    if (io->inference) return fail("%s: inference != 0 is refused -- a forward that is never differentiated over a shared encoding is vsl_encode_video + vsl_localize", who);
    if (io->sample_offset) return fail("%s: sample_offset=%d is refused: data parallel is not supported through a shared encoding", who, io->sample_offset);
    if (io->early_grads_event) return fail("%s: early_grads_event is refused: data parallel is not supported through a shared encoding", who);
    return 0;
}

// what refuses an ordinary backward (`who` = vsl_backward, or vsl_backward_accumulate without a vsl_shared_io): the last forward saved nothing, or
// it was a shared one
static int check_ordinary_saves(vsl_handle_s* h, const vsl_io* io, const char* who) {
    if (io->inference || io->workspace == h->infer_ws)
        return fail("%s: the last forward saved nothing (inference mode): run vsl_forward with inference = 0 for a batch that is to be differentiated", who);
    if (h->last_fwd == vsl_handle_s::FwdShared)
        return fail("%s: the handle's last forward was vsl_forward_shared: its saves are differentiated by vsl_backward_shared", who);
    return 0;
}

// the same for the backward of a shared step (vsl_backward_shared, or vsl_backward_accumulate with a vsl_shared_io)
static int check_shared_saves(vsl_handle_s* h, const vsl_io* io, const vsl_shared_io* sh, const char* who) {
    if (int rc = check_shared_io(io, sh, who)) return rc;
    if (h->last_fwd != vsl_handle_s::FwdShared || io->workspace == h->infer_ws)
        return fail("%s: the handle's last forward was not vsl_forward_shared (an ordinary forward is differentiated by vsl_backward; an inference forward saved nothing)", who);
    if (sh->N != h->shared_N) return fail("%s: N=%d, but the last vsl_forward_shared ran over N=%d videos", who, sh->N, h->shared_N);
    return 0;
}

// the body the three backward entry points share behind their own refusals (sh != nullptr: a shared step ; accumulate: vsl_backward_accumulate)
static int backward(vsl_handle_s* h, const vsl_io* io, const vsl_shared_io* sh, void* hip_stream, const char* who, bool accumulate = false) {
    if (int rc = check_backward_io(h, io, who)) return rc;
    Plan* p = nullptr;
    if (int rc = enqueue(h, io, sh ? PlanKind::TrainShared : PlanKind::Train, sh, hip_stream, vsl_handle_s::FwdNone, [&](Ctx& c) {
            c.accumulate = accumulate;
            run_backward(c);
            p = c.p;
        })) return rc;
    // (after an accumulating call too: the reduction recorded the squares of the values it STORED, so they describe the bucket as it now is)
    h->sq_src = p->sq_cover ? p->sq_dev : nullptr; h->sq_n = p->nblocks; h->sq_grads = io->grads;
    h->bwd_ws = io->workspace; h->bwd_stepped = io->fused_step != nullptr;
    return 0;
}

// what vsl_localize_pairs and vsl_highlight_pairs (`who`) refuse alike: the shape and the two resident encodings with their masks and indices
static int check_pairs_io(const vsl_pairs_io* l, const char* who) {
    if (l->B < 1) return fail("%s: B=%d pairs (at least one)", who, l->B);
    if (l->N < 1) return fail("%s: N=%d videos in the encoding (at least one)", who, l->N);
    if (l->Q < 1) return fail("%s: Q=%d queries in the encoding (at least one)", who, l->Q);
    if (l->Lq > MAX_LQ) return fail("%s: Lq=%d > %d query words", who, l->Lq, MAX_LQ);
    if (l->T > MAX_L) return fail("%s: T=%d > %d clips", who, l->T, MAX_L);
    if (!l->video_encoding) return fail("%s: video_encoding is NULL (the output of vsl_encode_video for the same T and params)", who);
    if (!l->query_encoding) return fail("%s: query_encoding is NULL (the output of vsl_encode_query for the same Lq and params)", who);
    if (!l->v_mask) return fail("%s: v_mask is NULL (the (N, T) clip mask of the video encoding)", who);
    if (!l->q_mask) return fail("%s: q_mask is NULL (the (Q, Lq) word mask of the query encoding)", who);
    if (!l->video_index) return fail("%s: video_index is NULL (the video of each pair)", who);
    if (!l->query_index) return fail("%s: query_index is NULL (the query of each pair)", who);
    return 0;
}

// what vsl_merge_topk and vsl_merge_windows (`who`; IO: vsl_merge_io / vsl_merge_windows_io) refuse alike: the shape and the lists they read
template <class IO>
static int check_merge_io(vsl_handle_s* h, const IO* io, const char* who) {
    if (!h || !io) return fail("%s: null argument", who);
    if (io->B < 1) return fail("%s: B=%d must be at least 1", who, io->B);
    if (io->G < 1) return fail("%s: G=%d must be at least 1", who, io->G);
    if (io->K < 1 || io->K > TOPK_MAX_K) return fail("%s: K=%d must be in [1, %d]", who, io->K, TOPK_MAX_K);
    if (io->K_out < 1 || io->K_out > TOPK_MAX_K) return fail("%s: K_out=%d must be in [1, %d]", who, io->K_out, TOPK_MAX_K);
    if (!io->start || !io->end || !io->score || !io->key || !io->count) return fail("%s: start, end, score, key and count are required inputs", who);
    if (!io->group_index) return fail("%s: null group_index", who);
    return 0;
}

// measuring switch of tools/merge_rate.py: the merge kernels without their cached heads
static bool merge_rescan_all() {
    static const bool on = getenv("VSL_MERGE_RESCAN_ALL") != nullptr;
    return on;
}

extern "C" {

int vsl_forward(vsl_handle h, const vsl_io* io, void* hip_stream) {
    if (int rc = check_io(h, io)) return rc;
    if (io->inference && io->training) return fail("vsl_forward: inference and training exclude each other (the inference kernels have no dropout)");
    if (io->inference) return enqueue(h, io, PlanKind::Infer, nullptr, hip_stream, vsl_handle_s::FwdInfer, forward_full);
    return enqueue(h, io, PlanKind::Train, nullptr, hip_stream, vsl_handle_s::FwdFull, forward_full);
}

// ---- training through a shared video encoding: N videos, B queries per step
int vsl_shared_workspace_floats(vsl_handle h, int B, int N, int T, int Lq, int Lc, int64_t* out) { return workspace_floats(h, PlanKind::TrainShared, B, T, Lq, Lc, out, N); }

int vsl_forward_shared(vsl_handle h, const vsl_io* io, const vsl_shared_io* sh, void* hip_stream) {
    if (int rc = check_io(h, io)) return rc;
    if (int rc = check_shared_io(io, sh, "vsl_forward_shared")) return rc;
    return enqueue(h, io, PlanKind::TrainShared, sh, hip_stream, vsl_handle_s::FwdShared, forward_full);
}

int vsl_backward_shared(vsl_handle h, const vsl_io* io, const vsl_shared_io* sh, void* hip_stream) {
    if (int rc = check_io(h, io)) return rc;
    if (int rc = check_shared_saves(h, io, sh, "vsl_backward_shared")) return rc;
    return backward(h, io, sh, hip_stream, "vsl_backward_shared");
}

// ---- one encoding per video, many queries against it (evaluation only: no dropout, nothing saved, no backward)
int vsl_encode_workspace_floats(vsl_handle h, int N, int T, int64_t* out) { return workspace_floats(h, PlanKind::Encode, N, T, 0, 0, out); }

int vsl_localize_workspace_floats(vsl_handle h, int B, int T, int Lq, int Lc, int64_t* out) { return workspace_floats(h, PlanKind::Localize, B, T, Lq, Lc, out); }

int vsl_encode_video(vsl_handle h, const vsl_encode_io* e, void* hip_stream) {
    if (!h || !e) return fail("null handle / io");
    if (e->N < 1) return fail("vsl_encode_video: N=%d videos (at least one)", e->N);
    if (!e->params || (!e->video_features && !e->video_features_bf16) || !e->v_mask || !e->video_encoding || !e->workspace)
        return fail("vsl_encode_io has a null device pointer");
    if (int rc = check_bf16_features(h, e->video_features_bf16)) return rc;
    vsl_io io = eval_io(e->N, e->T, 0, 0, e->params, e->workspace);
    io.video_features = e->video_features; io.video_features_bf16 = e->video_features_bf16; io.v_mask = e->v_mask;
    // (FwdInfer: nothing saved -- vsl_backward in this workspace and vsl_workspace_offset are refused as after an inference forward)
    return enqueue(h, &io, PlanKind::Encode, nullptr, hip_stream, vsl_handle_s::FwdInfer, [&](Ctx& c) { forward_encode(c, e->video_encoding); });
}

int vsl_localize(vsl_handle h, const vsl_localize_io* l, void* hip_stream) {
    if (!h || !l) return fail("null handle / io");
    if (l->B < 1) return fail("vsl_localize: B=%d queries (at least one)", l->B);
    if (l->N < 1) return fail("vsl_localize: N=%d videos in the encoding (at least one)", l->N);
    if (!l->video_encoding) return fail("vsl_localize: video_encoding is NULL (the output of vsl_encode_video for the same T and params)");
    if (!l->video_index) return fail("vsl_localize: video_index is NULL (the video of each query)");
    if (!l->v_mask) return fail("vsl_localize: v_mask is NULL (the (N, T) clip mask of the encoding)");
    if (!l->params || (!h->cfg.word_table && (!l->pad_vec || !l->glove_vec)) || !l->word_ids || !l->char_ids || !l->q_mask || !l->h_score || !l->start_logits ||
        !l->end_logits || !l->workspace)
        return fail("vsl_localize_io has a null device pointer");
    vsl_io io = eval_io(l->B, l->T, l->Lq, l->Lc, l->params, l->workspace);
    io.pad_vec = l->pad_vec; io.glove_vec = l->glove_vec;
    io.word_ids = l->word_ids; io.char_ids = l->char_ids; io.q_mask = l->q_mask;
    io.h_score = l->h_score; io.start_logits = l->start_logits; io.end_logits = l->end_logits;
    return enqueue(h, &io, PlanKind::Localize, nullptr, hip_stream, vsl_handle_s::FwdInfer, [&](Ctx& c) {
        io.v_mask = c.W(c.p->vmask);          // every kernel behind the join reads the gathered (B, T) mask
        forward_localize(c, CqContext{l->video_encoding, l->video_index}, l->v_mask);
    });
}

// ---- windows over a long video: each clip projected once, each window encoded (evaluation only, like vsl_encode_video)
int vsl_encode_windows_workspace_floats(vsl_handle h, int N, int T, int rows, int64_t* out) { return workspace_floats(h, PlanKind::EncodeWindows, N, T, 0, 0, out, rows); }

int vsl_encode_windows(vsl_handle h, const vsl_encode_windows_io* e, void* hip_stream) {
    if (!h || !e) return fail("null handle / io");
    if (!e->params || (!e->video_features && !e->video_features_bf16) || !e->video_encoding || !e->v_mask || !e->workspace)
        return fail("vsl_encode_windows_io has a null device pointer");
    if (!e->window_row) return fail("vsl_encode_windows: window_row is NULL (the first feature row of each window)");
    if (!e->window_len) return fail("vsl_encode_windows: window_len is NULL (the valid clips of each window)");
    if (int rc = check_bf16_features(h, e->video_features_bf16)) return rc;
    vsl_io io = eval_io(e->N, e->T, 0, 0, e->params, e->workspace);
    io.video_features = e->video_features; io.video_features_bf16 = e->video_features_bf16; io.v_mask = e->v_mask;
    // (the shape's refusals, by name: build_windows_plan.  FwdInfer: nothing saved -- vsl_backward in this workspace and vsl_workspace_offset are
    // refused as after an inference forward)
    return enqueue(h, &io, PlanKind::EncodeWindows, nullptr, hip_stream, vsl_handle_s::FwdInfer,
                   [&](Ctx& c) { forward_encode_windows(c, e->window_row, e->window_len, e->v_mask, e->video_encoding); }, e->rows);
}

// ---- one encoding per query, to be asked about many videos (evaluation only, like vsl_encode_video)
int vsl_encode_query_workspace_floats(vsl_handle h, int Q, int Lq, int Lc, int64_t* out) { return workspace_floats(h, PlanKind::EncodeQuery, Q, 0, Lq, Lc, out); }

int vsl_encode_query(vsl_handle h, const vsl_encode_query_io* e, void* hip_stream) {
    if (!h || !e) return fail("null handle / io");
    if (e->Q < 1) return fail("vsl_encode_query: Q=%d queries (at least one)", e->Q);
    if (!e->params || (!h->cfg.word_table && (!e->pad_vec || !e->glove_vec)) || !e->word_ids || !e->char_ids || !e->q_mask || !e->query_encoding || !e->workspace)
        return fail("vsl_encode_query_io has a null device pointer");
    vsl_io io = eval_io(e->Q, 0, e->Lq, e->Lc, e->params, e->workspace);
    io.pad_vec = e->pad_vec; io.glove_vec = e->glove_vec;
    io.word_ids = e->word_ids; io.char_ids = e->char_ids; io.q_mask = e->q_mask;
    // (FwdInfer: nothing saved -- vsl_backward in this workspace and vsl_workspace_offset are refused as after an inference forward)
    return enqueue(h, &io, PlanKind::EncodeQuery, nullptr, hip_stream, vsl_handle_s::FwdInfer, [&](Ctx& c) { forward_encode_query(c, e->query_encoding); });
}

// ---- pairs of resident encodings: vsl_localize with no query branch at all
constexpr int PAIRS_PLAN_LC = 4;      // the pairs plan has no embedding: its key carries the smallest legal Lc

int vsl_pairs_workspace_floats(vsl_handle h, int B, int T, int Lq, int64_t* out) { return workspace_floats(h, PlanKind::LocalizePairs, B, T, Lq, PAIRS_PLAN_LC, out); }

int vsl_localize_pairs(vsl_handle h, const vsl_pairs_io* l, void* hip_stream) {
    if (!h || !l) return fail("null handle / io");
    if (int rc = check_pairs_io(l, "vsl_localize_pairs")) return rc;
    if (!l->params || !l->h_score || !l->start_logits || !l->end_logits || !l->workspace) return fail("vsl_pairs_io has a null device pointer");
    vsl_io io = eval_io(l->B, l->T, l->Lq, PAIRS_PLAN_LC, l->params, l->workspace);
    io.h_score = l->h_score; io.start_logits = l->start_logits; io.end_logits = l->end_logits;
    return enqueue(h, &io, PlanKind::LocalizePairs, nullptr, hip_stream, vsl_handle_s::FwdInfer, [&](Ctx& c) {
        io.v_mask = c.W(c.p->vmask);          // every kernel behind the join reads the gathered (B, T) mask
        forward_pairs(c, CqContext{l->video_encoding, l->video_index, l->query_encoding, l->q_mask, l->query_index}, l->v_mask);
    });
}

// ---- the coarse half of a corpus search: vsl_localize_pairs up to the highlight score, one relevance per pair
int vsl_highlight_pairs(vsl_handle h, const vsl_highlight_io* r, void* hip_stream) {
    if (!h || !r) return fail("null handle / io");
    const vsl_pairs_io* l = &r->pairs;
    if (int rc = check_pairs_io(l, "vsl_highlight_pairs")) return rc;
    if (!l->params || !l->workspace) return fail("vsl_highlight_io has a null device pointer");
    if (r->relevance != 0 && r->relevance != 1) return fail("vsl_highlight_pairs: relevance=%d must be 0 (max) or 1 (mean)", r->relevance);
    if (!r->out) return fail("vsl_highlight_pairs: out is NULL (the relevance of each pair)");
    if (r->ld < 0 || (r->ld > 0 && r->ld < l->N))
        return fail("vsl_highlight_pairs: ld=%d must be 0 (out is (B)) or at least N=%d (out is a (Q, ld) matrix)", r->ld, l->N);
    vsl_io io = eval_io(l->B, l->T, l->Lq, PAIRS_PLAN_LC, l->params, l->workspace);
    return enqueue(h, &io, PlanKind::LocalizePairs, nullptr, hip_stream, vsl_handle_s::FwdInfer, [&](Ctx& c) {
        io.v_mask = c.W(c.p->vmask);          // every kernel behind the join reads the gathered (B, T) mask
        io.h_score = l->h_score ? l->h_score : c.W(c.p->p1.out);      // (no predictor runs: the first pass' output slot, (B T, 128), is free)
        forward_highlight(c, CqContext{l->video_encoding, l->video_index, l->query_encoding, l->q_mask, l->query_index}, l->v_mask, r->out, r->ld, r->relevance);
    });
}

int vsl_select_topm(vsl_handle h, const vsl_select_io* io, void* hip_stream) {
    if (!h || !io) return fail("vsl_select_topm: null argument");
    if (io->G < 1) return fail("vsl_select_topm: G=%d must be at least 1", io->G);
    if (io->N < 1) return fail("vsl_select_topm: N=%d must be at least 1", io->N);
    if (io->M < 1 || io->M > TOPM_MAX_M) return fail("vsl_select_topm: M=%d must be in [1, %d]", io->M, TOPM_MAX_M);
    if (io->ld < io->N) return fail("vsl_select_topm: ld=%d must be at least N=%d", io->ld, io->N);
    if ((int64_t)io->G * io->ld >= (int64_t(1) << 31)) return fail("vsl_select_topm: G * ld = %lld must stay below 2^31", (long long)io->G * io->ld);
    if (!io->key) return fail("vsl_select_topm: key is NULL (the (G, N) keys)");
    if (!io->out_index || !io->out_key || !io->out_count) return fail("vsl_select_topm: out_index, out_key and out_count are required outputs");
    launch_select_topm(SelectArgs{io->key, io->G, io->N, io->ld, io->M, io->out_index, io->out_key, io->out_count}, (hipStream_t)hip_stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int vsl_loss(vsl_handle h, const vsl_io* io, const vsl_loss_io* l, void* hip_stream) {
    if (!h || !io || !l) return fail("null argument");
    if (!l->start_labels || !l->end_labels || !l->h_labels || !l->losses) return fail("vsl_loss_io has a null pointer");
    if ((l->d_h_score == nullptr) != (l->d_start_logits == nullptr) || (l->d_h_score == nullptr) != (l->d_end_logits == nullptr))
        return fail("gradient seed outputs must be all set or all null");
    Plan* p = nullptr;
    const bool shared = !io->inference && h->last_fwd == vsl_handle_s::FwdShared;      // (the outputs of vsl_forward_shared: vsl_io.v_mask is the (B, T) per-query mask)
    if (int rc = get_plan(h, io->B, io->T, io->Lq, io->Lc, &p, io->inference ? PlanKind::Infer : shared ? PlanKind::TrainShared : PlanKind::Train, h->shared_N)) return rc;      // (its scratch lies where that forward's plan put it)
    ProfScope ps(h, "loss");
    launch_loss(LossArgs{io->start_logits, io->end_logits, io->h_score, l->start_labels, l->end_labels, l->h_labels, io->v_mask, io->B, io->T, l->inv_batch,
                         l->mask_sum, l->w_loc, l->w_highlight, io->workspace + p->loss_scratch, l->losses, l->d_start_logits, l->d_end_logits, l->d_h_score,
                         h->loss_counter}, (hipStream_t)hip_stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int vsl_group_loss_scratch_floats(int B, int G, int64_t* out) {
    if (!out) return fail("vsl_group_loss_scratch_floats: null argument");
    if (B < 1) return fail("vsl_group_loss_scratch_floats: B=%d must be at least 1", B);
    if (G < 1 || G > B) return fail("vsl_group_loss_scratch_floats: G=%d must be in [1, B=%d]", G, B);
    *out = group_loss_scratch_floats(B, G);
    return 0;
}

int vsl_group_loss(vsl_handle h, const vsl_group_loss_io* l, void* hip_stream) {
    if (!h || !l) return fail("vsl_group_loss: null argument");
    if (l->B < 1 || l->B > 65535) return fail("vsl_group_loss: B=%d must be in [1, 65535]", l->B);
    if (l->T < 1 || l->T > MAX_L) return fail("vsl_group_loss: T=%d must be in [1, %d]", l->T, MAX_L);
    if (l->G < 1 || l->G > l->B) return fail("vsl_group_loss: G=%d must be in [1, B=%d] (every group has at least one row)", l->G, l->B);
    if (!l->h_score || !l->start_logits || !l->end_logits || !l->v_mask)
        return fail("vsl_group_loss: h_score, start_logits, end_logits and v_mask are required inputs");
    if (!l->group_start || !l->positive) return fail("vsl_group_loss: group_start and positive are required inputs");
    if (!l->losses) return fail("vsl_group_loss: losses is NULL (the 5 output floats)");
    if (!l->scratch) return fail("vsl_group_loss: scratch is NULL (vsl_group_loss_scratch_floats(B, G) floats)");
    if ((l->d_h_score == nullptr) != (l->d_start_logits == nullptr) || (l->d_h_score == nullptr) != (l->d_end_logits == nullptr))
        return fail("vsl_group_loss: gradient seed outputs must be all set or all null");
    if (!(l->inv_temperature > 0.f)) return fail("vsl_group_loss: inv_temperature=%g must be positive", (double)l->inv_temperature);
    if (l->relevance != 0 && l->relevance != 1) return fail("vsl_group_loss: relevance=%d must be 0 (max) or 1 (mean)", l->relevance);
    if ((l->start_labels == nullptr) != (l->end_labels == nullptr)) return fail("vsl_group_loss: start_labels and end_labels must be both set or both null");
    if (!l->start_labels && l->w_loc != 0.f) return fail("vsl_group_loss: start_labels / end_labels are NULL but w_loc=%g is not 0", (double)l->w_loc);
    if (!l->h_labels && l->w_highlight != 0.f) return fail("vsl_group_loss: h_labels is NULL but w_highlight=%g is not 0", (double)l->w_highlight);
    const GroupLossArgs a{l->start_logits, l->end_logits, l->h_score, l->start_labels, l->end_labels, l->h_labels, l->v_mask, l->group_start, l->positive,
                          l->B, l->T, l->G, l->inv_pos, l->inv_groups, l->mask_sum, l->w_loc, l->w_highlight, l->w_rank, l->inv_temperature, l->relevance,
                          l->scratch, l->losses, l->hits, l->pair_relevance, l->d_start_logits, l->d_end_logits, l->d_h_score};
    { ProfScope ps(h, "group_loss_a"); launch_group_loss_a(a, (hipStream_t)hip_stream); }
    { ProfScope ps(h, "group_loss_c"); launch_group_loss_c(a, (hipStream_t)hip_stream); }
    HIP_OK(hipGetLastError());
    return 0;
}

int vsl_backward(vsl_handle h, const vsl_io* io, void* hip_stream) {
    if (int rc = check_io(h, io)) return rc;
    if (int rc = check_ordinary_saves(h, io, "vsl_backward")) return rc;
    return backward(h, io, nullptr, hip_stream, "vsl_backward");
}

// gradient accumulation: the same backward, whose writers of the bucket add to it (sh = NULL after vsl_forward, the step's vsl_shared_io after vsl_forward_shared)
int vsl_backward_accumulate(vsl_handle h, const vsl_io* io, const vsl_shared_io* sh, void* hip_stream) {
    if (int rc = check_io(h, io)) return rc;
    if (!io->grads) return fail("vsl_backward_accumulate needs grads: the bucket that holds the running sum");
    if (int rc = sh ? check_shared_saves(h, io, sh, "vsl_backward_accumulate") : check_ordinary_saves(h, io, "vsl_backward_accumulate")) return rc;
    return backward(h, io, sh, hip_stream, "vsl_backward_accumulate", true);
}

// the gradient with respect to the video features, behind a backward of the same io: one launch (backward.hip run_input_grads)
int vsl_input_grads(vsl_handle h, const vsl_io* io, const vsl_shared_io* sh, float* d_video_features, void* hip_stream) {
    if (int rc = check_io(h, io)) return rc;
    if (!d_video_features) return fail("vsl_input_grads: d_video_features is NULL (the (B, T, video_feature_dim) output; (N, T, video_feature_dim) after a shared step)");
    if (int rc = sh ? check_shared_saves(h, io, sh, "vsl_input_grads") : check_ordinary_saves(h, io, "vsl_input_grads")) return rc;
    if (!h->bwd_ws)
        return fail("vsl_input_grads: no backward has run since the handle's last forward: the gradient of VisualProjection's output is not there yet "
                    "(call vsl_backward, vsl_backward_shared or vsl_backward_accumulate on this io first)");
    if (h->bwd_ws != io->workspace) return fail("vsl_input_grads: vsl_io.workspace is not the workspace the last backward ran in");
    if (h->bwd_stepped)
        return fail("vsl_input_grads: the last backward applied fused_step: VisualProjection's weight has been overwritten by the update.  Run the "
                    "backward without fused_step, then vsl_input_grads, then vsl_adamw_step");
    return enqueue(h, io, sh ? PlanKind::TrainShared : PlanKind::Train, sh, hip_stream, vsl_handle_s::FwdNone, [&](Ctx& c) { run_input_grads(c, d_video_features); });
}

int vsl_abi_version(void) { return VSL_ABI_VERSION; }

uint64_t vsl_debug_rnn_launches(uint64_t n) { return (uint64_t)g_rnn_launches.exchange((unsigned long long)n); }

int64_t vsl_early_grad_offset(vsl_handle h) {
    if (!h) return -1;
    if (h->cfg.predictor != 1) return h->param_floats;
    int64_t off = h->param_floats;
    for (const ParamInfo& pi : h->params)
        if (pi.name.rfind("predictor.", 0) == 0) off = std::min<int64_t>(off, pi.off);
    return off;
}

int vsl_extract_index(vsl_handle h, const float* start_logits, const float* end_logits, int B, int T, int64_t* start_index,
                      int64_t* end_index, void* hip_stream) {
    if (!h || !start_logits || !end_logits || !start_index || !end_index) return fail("null argument");
    if (T > 8192) return fail("T too large");
    launch_extract_index(start_logits, end_logits, start_index, end_index, B, T, (hipStream_t)hip_stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int vsl_extract_topk(vsl_handle h, const vsl_topk_io* io, void* hip_stream) {
    if (!h || !io) return fail("vsl_extract_topk: null argument");
    if (!io->start_logits || !io->end_logits) return fail("vsl_extract_topk: null logits");
    if (io->B < 1) return fail("vsl_extract_topk: B=%d must be at least 1", io->B);
    if (io->T < 1 || io->T > MAX_L) return fail("vsl_extract_topk: T=%d must be in [1, %d]", io->T, MAX_L);
    if (io->K < 1 || io->K > TOPK_MAX_K) return fail("vsl_extract_topk: K=%d must be in [1, %d]", io->K, TOPK_MAX_K);
    if (io->max_span < 0) return fail("vsl_extract_topk: max_span=%d must be >= 0 (0 = unlimited)", io->max_span);
    if (!(io->nms_iou >= 0.f && io->nms_iou <= 1.f)) return fail("vsl_extract_topk: nms_iou=%g must be in [0, 1]", (double)io->nms_iou);
    if (!io->start_index || !io->end_index || !io->score) return fail("vsl_extract_topk: start_index, end_index and score are required outputs");
    launch_extract_topk(TopkArgs{io->start_logits, io->end_logits, io->valid_len, io->B, io->T, io->K, io->nms_iou, io->max_span, io->start_index,
                                 io->end_index, io->score, io->prob, io->count}, (hipStream_t)hip_stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int vsl_merge_topk(vsl_handle h, const vsl_merge_io* io, void* hip_stream) {
    if (int rc = check_merge_io(h, io, "vsl_merge_topk")) return rc;
    if (io->tag_per_slot && !io->tag) return fail("vsl_merge_topk: tag_per_slot needs a (B, K) tag");
    if (!io->out_tag || !io->out_list || !io->out_start || !io->out_end || !io->out_score || !io->out_key || !io->out_count)
        return fail("vsl_merge_topk: out_tag, out_list, out_start, out_end, out_score, out_key and out_count are required outputs");
    launch_merge_topk(MergeArgs{io->start, io->end, io->score, io->key, io->count, io->group_index, io->tag, io->B, io->K, io->G, io->K_out,
                                io->tag_per_slot != 0, merge_rescan_all(), io->out_tag, io->out_list, io->out_start, io->out_end, io->out_score, io->out_key,
                                io->out_count}, (hipStream_t)hip_stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int vsl_merge_windows(vsl_handle h, const vsl_merge_windows_io* io, void* hip_stream) {
    if (int rc = check_merge_io(h, io, "vsl_merge_windows")) return rc;
    if (!(io->nms_iou >= 0.f && io->nms_iou <= 1.f)) return fail("vsl_merge_windows: nms_iou=%g must be in [0, 1]", (double)io->nms_iou);
    if (!io->out_list || !io->out_start || !io->out_end || !io->out_score || !io->out_key || !io->out_count)
        return fail("vsl_merge_windows: out_list, out_start, out_end, out_score, out_key and out_count are required outputs");
    launch_merge_windows(MergeWindowsArgs{io->start, io->end, io->score, io->key, io->count, io->group_index, io->offset, io->B, io->K, io->G, io->K_out,
                                          io->nms_iou, merge_rescan_all(), io->out_list, io->out_start, io->out_end, io->out_score, io->out_key, io->out_count},
                         (hipStream_t)hip_stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int vsl_adamw_step(vsl_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const vsl_adamw* hp,
                   float* grad_norm_out, void* hip_stream) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || !hp) return fail("vsl_adamw_step: null argument");
    if (hp->step < 1) return fail("vsl_adamw_step: step must be >= 1 (got %d)", hp->step);
    if (int rc = ensure_opt_state(h)) return rc;
    const double bc1 = 1.0 - std::pow((double)hp->beta1, (double)hp->step), bc2 = 1.0 - std::pow((double)hp->beta2, (double)hp->step);
    const float* sq = nullptr;
    if (hp->norm_from_backward) {
        if (h->sq_grads != grads) return fail("vsl_adamw_step: norm_from_backward is set but `grads` is not the bucket the last vsl_backward wrote");
        sq = h->sq_src;             // (null when some gradient of this configuration does not leave k_reduce: the k_sqsum pass then)
    }
    ProfScope ps(h, "adamw");
    launch_adamw(AdamwArgs{params, grads, exp_avg, exp_avg_sq, h->decay_dev, h->opt_scratch, h->param_floats, hp->clip_norm,
                           AdamHp{hp->lr, hp->beta1, hp->beta2, hp->eps, hp->weight_decay, (float)bc1, (float)std::sqrt(bc2), hp->hf_order}, grad_norm_out, sq,
                           h->sq_n}, (hipStream_t)hip_stream);
    if (hipGetLastError() != hipSuccess) return fail("vsl_adamw_step: launch failed");
    return 0;
}


}  // extern "C"
