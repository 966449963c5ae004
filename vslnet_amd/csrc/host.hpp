// What the host units of libvslnet_hip.so share: the handle, the parameter / pack layout, the per-shape plan, the context of one call (Ctx) and the
// prototypes of what the units call across.  Host code only.
#pragma once
#include "../../include/vslnet_hip.h"
#include "launch.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

struct vsl_handle_s;

namespace vsl {

// the calling thread's state (streams.hip): the text vsl_last_error returns, and the handle whose call is enqueuing kernels on this thread (set for
// the duration of vsl_forward / vsl_backward)
extern thread_local std::string g_err;
extern thread_local vsl_handle_s* g_cur;
int fail(const char* fmt, ...);
#define HIP_OK(x)                                                                         \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) return fail("%s failed: %s", #x, hipGetErrorString(e_));    \
    } while (0)

struct ParamInfo { std::string name; int64_t off, numel; int ndim; int64_t dims[4]; };

struct EncP { int pos, dw[4], pw[4], pwb[4], lng[4], lnb[4], qw, qb, kw, kb, vw, vb, ln1g, ln1b, ln2g, ln2b, ow, ob; };
struct EncPk { int pw_f[4], pw_t[4], qkv_f, qkv_t, o_f, o_t; int pw_f3[4], pw_t3[4], qkv_f3, qkv_t3, o_f3, o_t3; };   // ..3: split packs
struct ModelP {
    int unk, char_tab, ccw[4], ccb[4], emb_w, emb_b, va_w, va_b;
    EncP fe;
    int w4C, w4Q, w4mlu, cqa_w, cqa_b, pool_w, cat_w, cat_b, hl_w, hl_b;
    EncP pe;
    int sln_g, sln_b, eln_g, eln_b, s0w, s0b, s1w, s1b, e0w, e0b, e1w, e1b;
    int l_wih[2], l_whh[2], l_bih[2], l_bhh[2];     // rnn predictor: start / end DynamicRNN (layers_t7.py:302-313)
};
struct ModelPk { int va_f, va_f16, va_f3, l_t3[2], emb_f, emb_t, emb_f3, emb_t3, emb_t3_cols; EncPk fe, pe; int cqa_f, cqa_t, cat1_f, cat1_t, s0_f, s0_t, e0_f, e0_t, ccw_img, ccw_imgb;
                 int l_f3[2], l_t[2], l_hf[2], l_hb[2], l_if, l_ib, zero128; };

// Workspace offsets (floats).  Every one defaults to -1 = "not part of this plan": a plan builder sets what its launch sequence uses and nothing else
// (Ctx::SV hands the kernels nullptr for the tensors only a backward reads).
struct EncWs {
    int64_t x0 = -1, y[4] = {-1, -1, -1, -1}, u[4] = {-1, -1, -1, -1}, mask[4] = {-1, -1, -1, -1}, h1 = -1, q = -1, k = -1, v = -1, lse = -1, att = -1, r = -1, h2 = -1, out = -1;
    int R = 0, L = 0;
};

// one DynamicRNN: x W_ih^T, activated gates, c_t, tanh(c_t), h_{t-1}, h * mask, gate grads, (B,2,128) dc/dh hand-over between time chunks
struct LstmWs { int64_t gi = -1, gates = -1, cseq = -1, tseq = -1, hprev = -1, out = -1, dG = -1, carry = -1; };

struct EncTmp { int64_t dr = -1, dq = -1, dk = -1, dv = -1, go = -1, gz[4] = {-1, -1, -1, -1}, ga = -1; };   // backward temporaries of one encoder application

struct SlabRec { int dst, n, nslabs, ss, rl, ds, vn; int64_t src; };

enum class PlanKind {
    Train,      // every save + the whole backward (build_train_plan)
    Infer,      // what a forward keeps live, reused by liveness (build_infer_plan)
    Encode,     // vsl_encode_video: B = videos, Lq = Lc = 0 (build_encode_plan)
    Localize,   // vsl_localize: the inference plan without the video pass
    LocalizePairs, // vsl_localize_pairs: the Localize plan without the query branch (no E, qf, qe, no embedding scratch)
    EncodeQuery,// vsl_encode_query: B = queries, T = 0: the packs and the query branch's own scratch (build_query_plan)
    TrainShared,// vsl_forward_shared / vsl_backward_shared: the training plan with the video half sized by N videos, everything else by B queries
    EncodeWindows // vsl_encode_windows: the Encode plan of (B = windows, T) + the (rows, 128) projection of the feature rows; rows sits in the key's N slot (build_windows_plan)
};

struct Plan {
    int B, T, Lq, Lc;
    int N = 0;                          // TrainShared: videos (VisualProjection + encoder application 0 run on N T rows); 0 = one video per sample
    int NV() const { return N > 0 ? N : B; }       // samples of the video half
    PlanKind kind = PlanKind::Train;
    int64_t vmask = -1;                 // Localize: the (N, T) clip mask gathered to (B, T)
    int rows = 0;                       // EncodeWindows: feature rows VisualProjection runs over
    int64_t wproj = -1;                 // EncodeWindows: its (rows, 128) output, which k_window_gather reads
    int64_t pack = -1, vf = -1, E = -1, argpos = -1, qf = -1;
    EncWs ve, qe, p1, p2;
    LstmWs lstm[2];
    int64_t h_gran = -1, gi_gran = -1, dg_gran = -1, dx_gran = -1;     // granule buffers of the fused rnn head (8 bytes per value); -1: chunked launches
    int64_t gran_floats = 0;                // their total extent (contiguous in the workspace, from h_gran)
    // epoch generation and workspace these buffers were last cleared for (rnn_granules_fresh): the last four workspaces, so that a caller who
    // alternates two or three of them (double buffering) does not pay a memset of the granule range in every forward
    struct GranSeen { const void* ws = nullptr; long long gen = -1; } gran_seen[4];
    int gran_next = 0;
    int64_t S = -1, Srow = -1, Scol = -1, M = -1, alpha = -1, pooled = -1, pb = -1, cat = -1, f1 = -1, f2 = -1, gated = -1, hid_s = -1, hid_e = -1, lnf_s = -1, lnf_e = -1;
    // backward temporaries
    int64_t loss_scratch = -1, gz_s = -1, gz_e = -1, dfeat_s = -1, dfeat_e = -1, dxh_s = -1, dxh_e = -1, g_s1 = -1, g_gated = -1;
    EncTmp tmp[4];                      // one set per encoder application: the applications' backward chains and their
                                        // weight-gradient launches overlap on different streams
    int64_t df2 = -1, df1 = -1, dC = -1, dSr = -1, dSs = -1, dQtot = -1, dvf = -1, dqf = -1, dE = -1, cqP1 = -1, cqP2 = -1, cqP3 = -1, cqP4 = -1, cqP5 = -1;
    int64_t dCv = -1, csr = -1;         // TrainShared: grad of the (N, T, 128) encoding ; the grouping as ints: start[N + 1], then members[B] from csr + csr_members()
    int64_t csr_members() const { return ((int64_t)NV() + 1 + 3) & ~int64_t(3); }
    int64_t partial = -1, partial_floats = 0, total = 0;      // the partial arena (offset, extent) ; the workspace's extent
    std::vector<int64_t> part_offs;     // sequence of partial-arena allocations made by the backward
    ReduceSeg* segs_dev = nullptr;
    int* blk2seg_dev = nullptr;         // block table: [early blocks | late blocks]
    float* sq_dev = nullptr;            // [nblocks] sum of squares of each reduction block's results (the clip's global norm, vsl_adamw.norm_from_backward)
    bool sq_cover = false;              // the reduction blocks write every element of the gradient bucket exactly once
    int nblocks = 0, nblocks_early = 0;
    uint64_t last_use = 0;              // LRU stamp of the plan cache (get_plan)
};

}  // namespace vsl

struct vsl_handle_s {
    vsl_config cfg;
    std::vector<vsl::ParamInfo> params;
    int64_t param_floats = 0;
    vsl::ModelP P;
    vsl::ModelPk K;
    int64_t pack_floats = 0;
    std::vector<vsl::PackJob> jobs;
    vsl::PackJob* jobs_dev = nullptr;
    int jobs_char = 0, jobs_first = 0, jobs_query = 0;  // jobs_dev = [char: the char-conv image embed_fwd reads | first: the video branch's opening kernels | query: the Embedding linear | everything else]
    int jobs_va = 0;                     // `first` = [the shared feature encoder's operands | these: VisualProjection's], so that vsl_localize packs [char | encoder] and vsl_encode_video `first` alone
    unsigned* loss_counter = nullptr;    // arrival counter of k_loss_fused (zero between calls)
    uint8_t* decay_dev = nullptr;        // per-element weight-decay flag of the flat bucket (vsl_adamw_step)
    float* opt_scratch = nullptr;        // OPT_BLOCKS partial sums of grads^2
    int cus = 0;                         // CUs of the device (vsl_create)
    const float* sq_src = nullptr;       // the last vsl_backward's per-block sums of squares (Plan::sq_dev), their count, the bucket they describe
    int sq_n = 0;
    const float* sq_grads = nullptr;
    std::map<std::tuple<int, int, int, int, int, vsl::PlanKind>, vsl::Plan*> plans;      // key: B, T, Lq, Lc, N (TrainShared; EncodeWindows: rows; 0 otherwise), kind
    // what the last forward left (api.hip record_forward):
    const void* infer_ws = nullptr;      // workspace the last INFERENCE forward ran in (it holds no saves: vsl_backward on it is refused) ; a training forward in it clears this
    enum LastFwd { FwdNone, FwdFull, FwdInfer, FwdShared };
    LastFwd last_fwd = FwdNone;          // its kind: vsl_backward / vsl_backward_shared refuse the other kind's saves, vsl_loss finds its scratch in that plan, and after
                                         // FwdInfer (inference forward, vsl_encode_video, vsl_localize, vsl_encode_query, vsl_localize_pairs) vsl_workspace_offset has nothing to point at
    int shared_N = 0;                    // N of the last vsl_forward_shared
    // what the backward entry points left since that forward (api.hip backward; cleared by record_forward): vsl_input_grads reads d_video_affine out
    // of the workspace and VisualProjection's weight out of vsl_io.params, so it needs a backward behind the forward, in that workspace, that has not
    // stepped the parameters
    const void* bwd_ws = nullptr;        // workspace of the last backward since the last forward (nullptr: none yet)
    bool bwd_stepped = false;            // ... and it applied vsl_io.fused_step
    uint64_t plan_clock = 0;
    // side streams for the independent chains (query branch, weight gradients) + fork/join events
    hipStream_t side[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> sync_pool;
    size_t sync_used = 0;
    // stop events riding on the kernel dispatches of the current call (launch.hpp VSL_LAUNCH); last one per stream
    std::vector<hipEvent_t> stop_pool;
    size_t stop_used = 0;
    bool stop_events = false;
    hipStream_t ev_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_last[4] = {nullptr, nullptr, nullptr, nullptr};
    int ev_n = 0;
    bool ev_dirty[4] = {false, false, false, false};     // a wait was enqueued on the stream AFTER its last kernel: that kernel's stop event no
                                                         // longer stands for "everything enqueued so far" (the shortcut is not transitive)
    hipEvent_t last_event(hipStream_t s) const {
        for (int i = 0; i < ev_n; ++i) if (ev_stream[i] == s) return ev_dirty[i] ? nullptr : ev_last[i];
        return nullptr;
    }
    void mark_waiting(hipStream_t s) { for (int i = 0; i < ev_n; ++i) if (ev_stream[i] == s) ev_dirty[i] = true; }
    bool multi_stream = true;
    // optional per-kernel timing with HIP events on the launch stream (vsl_profile_*), used by bench.py's roofline line
    bool prof_on = false;
    std::string prof_sel;
    std::vector<hipEvent_t> prof_pool;
    size_t prof_used = 0;
    struct ProfRec { const char* name; size_t e0, e1; hipStream_t s; double host_us; int deps[6]; int nd; };
    std::vector<ProfRec> prof_recs;
    const char* prof_name = nullptr;     // name of the LAUNCH being enqueued when it is profiled (vsl_launch_events)
    // dependency bookkeeping of the critical-path ledger (vsl_profile_launch): last profiled launch per stream, and the cross-stream
    // ordering points (Ctx::order) enqueued since -- they become `deps` of the consumer stream's next launch
    std::vector<std::pair<hipStream_t, int>> prof_last, prof_pending;
    std::chrono::steady_clock::time_point prof_t0;
    void prof_wait(hipStream_t from, hipStream_t to) {
        if (!prof_on || from == to) return;
        for (auto& kv : prof_last) if (kv.first == from) { prof_pending.push_back({to, kv.second}); return; }
    }
};

namespace vsl {

// the bookkeeping of one enqueuing call (vsl_forward / vsl_backward / ...): event pools rewound, the handle published to vsl_launch_events
struct CallScope {
    explicit CallScope(vsl_handle_s* h);
    ~CallScope();
};

// vsl_loss / vsl_adamw_step: plain launches on the caller's stream; when the built-in profiler selects `name` they carry timing events too
struct ProfScope {
    vsl_handle_s* h;
    ProfScope(vsl_handle_s* h_, const char* name);
    ~ProfScope();
};

struct Ctx {
    vsl_handle_s* h;
    Plan* p;
    const vsl_io* io;
    hipStream_t s;
    // Plan-building pass (build_train_plan runs run_backward once per plan, with io == nullptr and ws == nullptr; a forward is never run dry): record
    // the partial-slab allocations, launch nothing.  Every pointer this struct hands out -- W, SV, P, PK, part_ptr, slab, the vsl_io accessors below --
    // is nullptr then, so no call site tests `dry` to form one.  What does test it is behaviour, not addressing: LAUNCH and order_n (nothing is
    // enqueued), part_alloc / reg / slab (record instead of replay), the backward's choice of streams and of deferring weight gradients (a dry run has
    // no streams), and the blocks that touch what has no null value to stand in for it: vsl_io.early_grads_event, and the process-wide tag counter of
    // the fused rnn launches.  (fused_loss / fused_step and their scalar fields sit behind fused_loss() / fused_step(), null in a dry run.)
    bool dry;
    float* ws;
    size_t part_idx = 0;
    int64_t part_cur = 0;
    std::vector<SlabRec>* recs = nullptr;
    const vsl_shared_io* sh = nullptr;  // vsl_forward_shared / vsl_backward_shared: the videos' index and clip mask (the plan is TrainShared then)
    bool accumulate = false;            // vsl_backward_accumulate: the writers of the gradient bucket (the two reductions, the trainable word table) add to it
    bool inf() const { return p->kind != PlanKind::Train && p->kind != PlanKind::TrainShared; }
    // a tensor only the backward reads: its address in a training forward, nullptr in an inference forward (the kernels then do not store it)
    float* SV(int64_t off) const { return dry || inf() ? nullptr : ws + off; }
    const float* P(int off) const { return dry ? nullptr : io->params + off; }
    const float* PK(int off) const { return dry ? nullptr : ws + p->pack + off; }
    float* W(int64_t off) const { return dry ? nullptr : ws + off; }
    // what the backward reads from the call's vsl_io (nullptr in a dry run: there is no call)
    const float* v_mask() const { return dry ? nullptr : io->v_mask; }      const float* q_mask() const { return dry ? nullptr : io->q_mask; }
    // the clip mask of the video half: (N, T) per video in a shared step, vsl_io.v_mask otherwise ; the shared step's video of each query
    const float* video_mask() const { return dry ? nullptr : sh ? sh->video_v_mask : io->v_mask; }
    const int* video_index() const { return dry || !sh ? nullptr : sh->video_index; }
    const int64_t* word_ids() const { return dry ? nullptr : io->word_ids; }  const int64_t* char_ids() const { return dry ? nullptr : io->char_ids; }
    const float* video_features() const { return dry ? nullptr : io->video_features; }
    const uint16_t* video_features_bf16() const { return dry ? nullptr : io->video_features_bf16; }
    float* h_score() const { return dry ? nullptr : io->h_score; }            float* grads() const { return dry ? nullptr : io->grads; }
    float* start_logits() const { return dry ? nullptr : io->start_logits; }  float* end_logits() const { return dry ? nullptr : io->end_logits; }
    // the loss seeds: the outputs of vsl_io.fused_loss when the loss is part of the call, the caller's otherwise
    const float* d_start_logits() const { return dry ? nullptr : io->fused_loss ? io->fused_loss->d_start_logits : io->d_start_logits; }
    const float* d_end_logits() const { return dry ? nullptr : io->fused_loss ? io->fused_loss->d_end_logits : io->d_end_logits; }
    const float* d_h_score() const { return dry ? nullptr : io->fused_loss ? io->fused_loss->d_h_score : io->d_h_score; }
    // the loss / the optimizer step inside the call (nullptr: not asked for, or a dry run)
    const vsl_loss_io* fused_loss() const { return dry ? nullptr : io->fused_loss; }   const vsl_fused_step* fused_step() const { return dry ? nullptr : io->fused_step; }
    // raw allocation in the partial arena
    int64_t part_alloc(int64_t n) {
        n = (n + 3) & ~int64_t(3);
        if (dry) { p->part_offs.push_back(part_cur); part_cur += n; return p->part_offs.back(); }
        return p->part_offs[part_idx++];
    }
    // register a reduction source: `src` is an ABSOLUTE workspace offset (partial arena or any saved buffer)
    void reg(int dst, int n, int64_t src, int nslabs, int ss, int rl = 0, int ds = 0, int vn = 0) {
        if (dry) recs->push_back(SlabRec{dst, n, nslabs, ss, rl ? rl : n, ds, vn ? vn : n, src});
    }
    // the common case: `nslabs` contiguous slabs of n floats for the parameter at dst
    float* slab(int dst, int n, int nslabs) {
        const int64_t o = part_alloc((int64_t)n * nslabs);
        reg(dst, n, p->partial + o, nslabs, n);
        return W(p->partial + o);
    }
    float* part_ptr(int64_t o) const { return W(p->partial + o); }
    // make stream `to` wait for everything enqueued so far on stream `from` ; order2: one event record on `from`, two waiters (streams.hip)
    void order(hipStream_t from, hipStream_t to) { order_n(from, &to, 1); }
    void order2(hipStream_t from, hipStream_t to1, hipStream_t to2) { const hipStream_t to[2] = {to1, to2}; order_n(from, to, 2); }
    void order_n(hipStream_t from, const hipStream_t* to, int n);
    hipStream_t side(int k) const { return (h->multi_stream && h->side[k]) ? h->side[k] : main; }
    hipStream_t main = nullptr;
    // built-in profiler: a selected LAUNCH hands its name to vsl_launch_events, which puts timing events on the kernel's own packet
    void pb(const char* name);           // prof_sel: "*", one launch name, or a comma-separated list of names (prof_selected)
    void pe() { h->prof_name = nullptr; }
    // elements one sample owns in the tensor dropped at `site` (the masks are keyed by the row-major element index)
    uint32_t site_elems(int site) const {
        const vsl_config& cf = h->cfg;
        const uint32_t T = p->T, Lq = p->Lq;
        if (site == 64) return T * cf.video_feature_dim;              // SITE_VIS
        if (site == 65) return Lq * cf.word_dim;                      // SITE_WORD
        if (site == 66) return Lq * p->Lc * cf.char_dim;              // SITE_CHAR
        if (site == 67) return T * D;                                 // SITE_CQ_C
        if (site == 68) return Lq * D;                                // SITE_CQ_Q
        const uint32_t L = (site >> 4) == 1 ? Lq : T;                 // encoder pass 1 = query
        if ((site & 15) != 5) return L * D;
        // 5 = attention probabilities (B, H, L, L); the kernels of L > 256 key their masks by key PAIRS (common.hpp drop_hash_odd): ceil(L / 2) hashes per row
        return L > 256 ? cf.num_heads * L * ((L + 1) / 2) : cf.num_heads * L * L;
    }
    Drop drop(int site) const {
        Drop d{0u, 0u, 1.0f, 0u};
        const float pr = h->cfg.drop_rate;
        if (io && io->training && pr > 0.f) {
            uint32_t x = (uint32_t)io->seed ^ ((uint32_t)(io->seed >> 32) * 0x9E3779B1u) ^ ((uint32_t)site * 0x85EBCA77u + 0x165667B1u);
            x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
            uint32_t k = x ^ 0x68E31DA4u;               // the site key: a second, independent hash of (step seed, site)
            k ^= k >> 15; k *= 0x2C1B3C6Du; k ^= k >> 12; k *= 0x297A2D39u; k ^= k >> 15;
            d.key = k;
            // keep = drop_hash(element, seed, key), element enters as element * 0x9E3779B1 + seed: a shard that starts at sample s of the global batch continues the
            // element counter at s * site_elems, which folds into the seed (no cost in the kernels)
            x += (uint32_t)io->sample_offset * site_elems(site) * 0x9E3779B1u;
            d.seed = x;
            d.thresh = (uint32_t)std::min(4294967295.0, (double)pr * 4294967296.0);
            d.scale = 1.0f / (1.0f - pr);
        }
        return d;
    }
};
#define LAUNCH(name, stmt) do { if (!c.dry) { c.pb(name); stmt; c.pe(); } } while (0)

// dropout site ids: encoder application `app` (0 video, 1 query, 2 predictor pass 1, 3 predictor pass 2) uses
// app * 16 + {0..3 conv layers, 4 LN1 out, 5 attention probs, 6 attention out, 7 LN2 out, 8 out_layer}
enum { SITE_VIS = 64, SITE_WORD = 65, SITE_CHAR = 66, SITE_CQ_C = 67, SITE_CQ_Q = 68 };

// ------------------------------------------------------------------------------------------------ what the units call across
// layout.hip
void build_params(vsl_handle_s* h);
void build_packs(vsl_handle_s* h);
void finish_pack_jobs(vsl_handle_s* h);
int ensure_opt_state(vsl_handle_s* h);
// plan.hip
int get_plan(vsl_handle_s* h, int B, int T, int Lq, int Lc, Plan** out, PlanKind kind = PlanKind::Train, int N = 0);     // N: TrainShared (videos) and EncodeWindows (feature rows) only
void free_plan(Plan* p);
// streams.hip
bool prof_selected(const vsl_handle_s* h, const char* name);
bool query_chain_is_longer(const Plan& p);      // after the backward's video / query fork
// forward.hip
// the operands of CQAttention: the context C (B, T, 128), or a resident (N, T, 128) encoding read through vidx (B); the encoded query Qf (B, Lq, 128) with its
// (B, Lq) mask -- nullptr: the plan's own query pass and vsl_io.q_mask -- or a resident (Q, Lq, 128) encoding and its (Q, Lq) mask read through qidx (B)
struct CqContext { const float* C; const int* vidx; const float* Qf = nullptr; const float* qmask = nullptr; const int* qidx = nullptr; };
void forward_full(Ctx& c);                      // vsl_forward, or (c.sh set, plan TrainShared) vsl_forward_shared
void forward_encode(Ctx& c, float* video_encoding);
void forward_encode_windows(Ctx& c, const int32_t* window_row, const int32_t* window_len, float* v_mask, float* video_encoding);
void forward_localize(Ctx& c, CqContext ctx, const float* vmask_nt);
void forward_encode_query(Ctx& c, float* query_encoding);
void forward_pairs(Ctx& c, CqContext ctx, const float* vmask_nt);
void forward_highlight(Ctx& c, CqContext ctx, const float* vmask_nt, float* out, int ld, int mean);      // vsl_highlight_pairs: forward_pairs up to cq_out + the relevance reduction
bool query_fused(const Ctx& c);
std::vector<int> lstm_chunks(int T);
extern std::atomic<unsigned long long> g_rnn_launches;
unsigned rnn_epoch(long long* gen = nullptr);
void rnn_granules_fresh(Ctx& c, Plan& p, long long gen);
// backward.hip
void run_backward(Ctx& c);                      // the ordinary step, or (plan TrainShared, c.sh set unless dry) the step through a shared encoding
void run_input_grads(Ctx& c, float* d_video_features);     // vsl_input_grads: one launch on c.s behind a backward of the same io

}  // namespace vsl
