// Host-side launcher prototypes + small POD argument structs shared by the kernel units (kernels_*.hip) and the host units (host.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "common.hpp"

namespace vsl {

struct PackJob {          // one weight -> packed B-operand copy (see common.hpp pack_index)
    int src;              // float offset into the flat parameter buffer
    int dst;              // float offset into the pack buffer
    int kn, cn;           // extent of the contraction index / of the output-column index covered by this job
    int ld;               // leading dimension of the source matrix
    int transpose;        // 0: Bm[k][c] = W[c][k] (forward pack)   1: Bm[k][c] = W[k][c] (data-gradient pack)  2: copy  3: char-conv image  4: zero fill  8: char-conv B-operand image of k_embed_bwd
                          // 9 / 10: W_hh (512, 128) in the register order of k_lstm1_fwd / k_lstm1_bwd (kn = 65536 floats)
                          // 5: bf16 forward pack   6 / 7: SPLIT packs (three bf16 planes h, m, l; common.hpp pack3_index) of the forward / data-gradient operand
    int ncols;            // total columns of the packed operand
    int k_off, col_off;   // placement inside the packed operand
    int ktot;             // split packs: contraction extent of the whole operand incl. padding (plane size); 0 = kn
    int kfill;            // split packs: k rows this job writes (rows >= kn as zeros); 0 = kn rounded up to 16
};

struct CharConvPtrs { const float* w[4]; const float* b[4]; };

struct HeadArgs {
    const float* feat;    // (R,128) encoder / rnn features
    const float* ln_g;    // nullptr for the rnn predictor
    const float* ln_b;
    const float* W0pack;  // forward pack of (128, 256)
    const float* b0;
    const float* w1;      // (128)
    const float* b1;      // (1)
    float* hid;           // (R,128) relu output, saved (nullable: an inference forward does not store it)
    float* lnfeat;        // (R,128) LN(feat), saved for the weight gradient (nullable)
    float* logits;        // (R)
};

struct HeadBwdArgs {
    const float* dlogit;  // (R)
    const float* hid;     // (R,128)
    const float* feat;    // (R,128)
    const float* ln_g;
    const float* W0Tpack; // transpose pack, ncols = 256
    const float* w1;
    float* gz;            // (R,128) grad wrt the pre-relu activation (G operand of the weight gradient)
    float* dfeat;         // (R,128)
    float* dx;            // (R,128) grad wrt the gated features through this head
    float* p_b0;          // partial slabs [ntiles][128]
    float* p_w1;          // [ntiles][128]
    float* p_b1;          // [ntiles]
    float* p_lng;         // [ntiles][128]
    float* p_lnb;         // [ntiles][128]
    // vsl_io.fused_loss, T >= 32 (a 32-row tile then touches at most two samples; ragged T included): the tile's seeds dlogit[r] = cs * (softmax(logits of r's sample)[t] - [t == label]) are computed HERE
    // (the CrossEntropy gradient needs nothing but the sample's own T logits), so the loss launch is not on the dependent chain; logits == nullptr: read dlogit
    const float* logits;  // (B, T)
    const int64_t* label; // (B)
    float cs;             // w_loc * inv_batch
    int T;
};

// generic weight-gradient job: dW[n][k] = sum_r G[r][n] * A[r][k]  over row chunks -> partial slabs
struct WgradJob {
    const float* G[3];    // N = 128 * nG ; each (R,128)
    const float* A[4];    // column blocks of 128 (ldA == 128 each) when nA > 0
    const float* Afull;   // or one (R, K) matrix with leading dimension K (nA == 0)
    int nG, nA, K;
    int R;
    int ldg;              // row stride of the G blocks in floats (0 = 128): the LSTM gate gradients are 512 wide
    int drop_on_A;        // apply dropout to Afull on load (VisualProjection input)
    int a_bf16;           // Afull points to bfloat16 data (bf16 throughput mode: the features), widened on load
    Drop dp;
    float* out;           // partial slabs [nchunk][N][K]
    float* out_bias[3];   // partial slabs [nchunk][128] per G block (nullable)
    int rows;             // rows per chunk = workgroup of THIS job (0 = WG_ROWS; a multiple of 16): see wgrad_rows_one_round
};
#ifndef VSL_WG_ROWS
#define VSL_WG_ROWS 256
#endif
constexpr int WG_ROWS = VSL_WG_ROWS;     // rows per weight-gradient chunk = workgroup (one partial slab each)
__host__ __device__ inline int wgrad_rows(const WgradJob& j) { return j.rows > 0 ? j.rows : WG_ROWS; }
__host__ __device__ inline int wgrad_chunks(int R, int rows) { return (R + rows - 1) / rows; }
// A batch of `cols` 128 x 128 output blocks over R rows that is launched into an EMPTY chip (the step's last weight-gradient batch) takes
// ceil(cols * chunks / CUs) rounds of one-workgroup-per-CU chunks: 384 workgroups of 256 rows are two rounds, the second half empty.  Longer chunks
// that make it whole rounds cost rows / 256 each: -> the smallest multiple of 16 rows >= WG_ROWS with cols * chunks <= CUs * floor(rounds at WG_ROWS).
inline int wgrad_rows_whole_rounds(int R, int cols, int cus) {
    const int wgs = cols * wgrad_chunks(R, WG_ROWS);
    if (cus <= 0 || cols <= 0 || wgs <= cus || wgs % cus == 0) return WG_ROWS;
    const int target = cus * (wgs / cus);
    for (int rows = WG_ROWS + 16; rows <= 4 * WG_ROWS; rows += 16)
        if (cols * wgrad_chunks(R, rows) <= target) return rows;
    return WG_ROWS;
}
constexpr int MAX_WJOBS = 12;
struct WgradBatch { WgradJob j[MAX_WJOBS]; int n; int start[MAX_WJOBS + 1]; };   // start: first workgroup of each job (launch_wgrad fills it)

struct ReduceSeg {        // grads[dst + (i / rl) * ds + i % rl] = sum over sources q, slabs s of partial[src[q] + s * ss[q] + i],  i < n
    int dst, n;
    int rl, ds;           // destination row length / row stride (rl == n, ds == 0 for a contiguous destination)
    int nsrc;
    int src[4], nslabs[4], ss[4]; // float offsets into the WORKSPACE (partial arena or any saved buffer), slab count, slab stride
    int vec;                      // 1: n, every src, ss and vn are multiples of 4 floats -> 16-byte loads/stores
    int vn[4];                    // source q contributes to elements i < vn[q] only (shorter sequences of a shared table)
};

// Opt a kernel into more than the default 64 KiB of dynamic LDS.  Requests exactly what the launch needs (static LDS
// counts against the same 160 KiB), grows monotonically, and reports -- instead of silently poisoning
// hipGetLastError() -- when the runtime refuses.
// Every kernel of a multi-stream step is launched with a STOP EVENT on its own dispatch packet (hipExtLaunchKernelGGL): a cross-stream
// ordering point is then a bare hipStreamWaitEvent on the producer's last kernel.  hipEventRecord puts a marker packet into the producer
// stream instead, which costs it 4-5 us per fork and 7 us more per join (tools/ubench/event_fork.hip: chain 21.6 / fork by record 26.9 /
// fork by stop event 23.3 / stop event on every dispatch, no waiter 21.6 us per link).  streams.hip hands out the events (none = plain launch).
// The same hook serves the built-in profiler (vsl_profile_select): a profiled launch gets a timing START and STOP event on its own packet, so
// the measured interval is the kernel's execution and the stream carries no extra marker packets.
void vsl_launch_events(hipStream_t s, hipEvent_t* start, hipEvent_t* stop);
#define VSL_LAUNCH(kernel, grid, block, shm, stream, ...)                                                                   \
    do {                                                                                                                   \
        hipEvent_t st__ = nullptr, sp__ = nullptr;                                                                         \
        vsl::vsl_launch_events(stream, &st__, &sp__);                                                                      \
        if (sp__) hipExtLaunchKernelGGL(kernel, grid, block, shm, stream, st__, sp__, 0, __VA_ARGS__);                     \
        else hipLaunchKernelGGL(kernel, grid, block, shm, stream, __VA_ARGS__);                                            \
    } while (0)

inline void ensure_dynamic_lds(const void* func, size_t bytes, size_t& granted, const char* name) {
    if (bytes <= granted || bytes <= 64 * 1024) return;
    const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        fprintf(stderr, "[vslnet_hip] hipFuncSetAttribute(%s, %zu B dynamic LDS) failed: %s\n", name, bytes, hipGetErrorString(e));
        (void)hipGetLastError();
    } else {
        granted = bytes;
    }
}
template <auto KERNEL> void dynamic_lds_optin(size_t bytes, const char* name) {      // (one grant per kernel instantiation)
    static size_t granted = 0;
    ensure_dynamic_lds((const void*)KERNEL, bytes, granted, name);
}

// ---------------------------------------------------------------- forward
void launch_pack(const float* params, float* pack, const PackJob* jobs_dev, int njobs, hipStream_t s);
// bf16 throughput mode: X bf16 (R, Dv), packed bf16 weight (PackJob type 5), fp32 accumulate / bias / output
void launch_vproj_fwd_bf16(const uint16_t* X, const uint16_t* Wpack16, const float* bias, float* Y, int R, int Dv, Drop dp, hipStream_t s);
// fp32-grade on the bf16 matrix cores (kernels_split.hip): W3 = split pack (PackJob type 6 / 7) of the (Dv, 128) operand
void launch_vproj_fwd3(const float* X, const uint16_t* W3, const float* bias, float* Y, int R, int Dv, Drop dp, hipStream_t s,
                       int seg = 0, int stride = 0, int off = 0);   // seg > 0: rows of one time chunk (see launch_linear_fwd3)
void launch_linear_fwd3(const float* A, const uint16_t* W3, const float* bias /* nullable */, float* Y, int R, int K, hipStream_t s, int ncols = 128,
                        int seg = 0, int stride = 0, int off = 0);      // ncols: columns of the operand and of Y's rows; seg > 0: rows of one time chunk of a (B, T, .) tensor
void launch_linear_bwd_data3(const float* G, const uint16_t* WT3, float* dA, int R, int K, int Kc, hipStream_t s);   // Kc: columns of the split pack
// word + character embedding of the query words (kernels_embed.hip)
struct EmbedFwdArgs {
    const int64_t *word_ids, *char_ids;   // (Rq), (Rq, Lc)
    const float *pad_vec, *unk_vec, *glove;   // rows 0, 1 and 2.. of the [pad; unk; glove] table (the caller's vectors, or the trainable word table's rows)
    const float* char_tab;
    CharConvPtrs cc;                      // the four char convs' weights and biases in the parameter buffer
    const float* wimg;                    // their weights as the [ci][4 taps][100 channels] image (PackJob type 3)
    float* E;                             // (Rq, word_dim + 100) out
    int8_t* argpos;                       // (Rq, 100) arg-max position per channel, saved (nullable: an inference forward does not store it)
    int Rq, Lc, word_dim, char_dim;
    Drop dw, dc;
};
void launch_embed_fwd(const EmbedFwdArgs& a, hipStream_t s);
// the Embedding linear at a width the split kernel's 16-wide K steps do not tile (kernels_embed.hip)
void launch_linear_fwd(const float* A, const float* Wpack, const float* bias, float* Y, int R, int K, hipStream_t s);
// LN1 + fused QKV projection at the end of the conv-block kernel (row-local on the owner rows)
struct QkvFuse {
    const float *ln_g, *ln_b, *bq, *bk, *bv;
    float *h1, *q, *k, *v;
    Drop d1;
};
// fused conv block of one encoder application (kernels_enc.hip): 4 layers + LN1 / QKV in one launch, 12-row recomputed halo
struct CbFwdArgs {
    const uint16_t* W3[4];         // split packs (PackJob type 6) of the four pointwise weights
    const uint16_t* Wqkv3;         // split pack of the fused (128, 384) QKV operand
    const float *xin, *pos;
    float* x0_out;
    const float *ln_g[4], *ln_b[4], *dw_w[4], *pw_b[4];
    float *y[4], *u[4];
    uint32_t* relu_mask[4];
    Drop dp[4];
    QkvFuse qf;
    int R, L;
    int nosave;                    // inference: the instantiation that stores y[3], q, k, v only (x0_out, y[0..2], u, relu_mask, qf.h1 may be null; no dropout)
};
void launch_convblock_fwd(const CbFwdArgs& a, hipStream_t s);
// the attention-output backward of one encoder application (a8 :183-190 backward; tile_bodies.hpp attn_out_bwd_tile)
struct AttnOutBwdArgs {
    const float *dy, *dy2, *r_in, *ln_g, *WTpack;
    float *g_o, *dr, *p_lng, *p_lnb;
    Drop d4, d5;
};
// gating + HighLightLayer + CQConcatenate backward of one 32-row tile (kernels_cq_bwd.hip k_cqcat_bwd / tile_bodies.hpp cqcat_bwd_tile)
struct CqcatBwdArgs {
    const float *dg0, *dg1, *dg2, *dh_loss, *f2, *hscore, *wh, *W1Tpack;
    float *df2, *df1, *p_wh, *p_bh;
    // vsl_io.fused_loss: the highlight loss' seed (elementwise: k_loss_fused's expression) computed in place of the dh_loss read; h_lab == nullptr: read dh_loss
    const int64_t* h_lab;
    const float* vmask;
    float w_hl, mask_sum;
};
// a8 backward, first half (k_qkv_bwd's work), hosted by the conv block's backward kernel on its 56-row window:
// dy = dr + LN1^T(([dQ | dK | dV] [Wq; Wk; Wv]) * m1) -- the conv block's incoming gradient never goes through memory
struct QkvBwdFuse {
    const float *dq, *dk, *dv;     // (R,128) each
    const float* x;                // (R,128) LN1 input = the conv block's output y3
    const float* dr;               // (R,128) gradient of the residual path (attention-output backward)
    const float* ln_g;             // LN1 gamma
    const uint16_t* WT3;           // split pack (type 7) of [Wq; Wk; Wv]: 384 contraction rows, 128 columns
    float *p_lng, *p_lnb;          // partial slabs [ntiles][128]
    Drop d1;
};
struct CbBwdArgs {
    const uint16_t* WT3[4];        // split packs (PackJob type 7) of the pointwise weights' data-gradient operand
    const float* dy;               // (R,128) grad wrt the block output (unused when qkv is set)
    const float* x[4];             // LayerNorm inputs of layers 0..3 (x0, y0, y1, y2)
    const uint32_t* relu_mask[4];
    const float *ln_g[4], *ln_b[4], *dw_w[4];
    Drop dp[4];
    float* gz[4];                  // out (R,128): dz per layer, G operand of the pointwise weight gradients
    float* dx0;                    // out (R,128): grad wrt the block input (x + pos)
    float *p_lng[4], *p_lnb[4], *p_dw[4];   // partial slabs [ntiles][128] / [ntiles][128 * 7]
    int R, L;
    // what the workgroup goes on with, on its own 32 rows of dx0 (1, 2: whole-tile instantiation only: convblock_bwd_hosts_tail):
    // 0 nothing ; 1 the attention-output backward of the encoder pass below (tail_ao; its dy = dx0) ; 2 the CQConcatenate backward (tail_cq; its dg0 = dx0)
    int tail;
    AttnOutBwdArgs tail_ao;
    CqcatBwdArgs tail_cq;
    // 3 (sample tiles only): the Embedding linear's data gradient dA (R, K) = dx0 WT3 -- the query pass' conv block goes on with k_linear_bwd_data3's work
    const uint16_t* tail_lin_WT3;  // split transpose pack, Kc >= K columns (a multiple of 512)
    float* tail_lin_dA;
    int tail_lin_K, tail_lin_Kc;
    int qkv;                       // 1: the workgroup first computes dy from qk (whole-tile instantiation only: convblock_bwd_hosts_tail)
    QkvBwdFuse qk;
};
void launch_convblock_bwd(const CbBwdArgs& a, hipStream_t s);
bool convblock_bwd_hosts_tail(int R, int L);      // does launch_convblock_bwd honour CbBwdArgs::tail for this shape?
bool convblock_bwd_hosts_linear(int R, int L);    // ... and tail 3 (the Embedding linear's data gradient)?
bool convblock_bwd_hosts_qkv(int R, int L);       // ... and CbBwdArgs::qkv?  (its LN1 partial slabs are then convblock_slabs(R, L) many)
int convblock_slabs(int R, int L);        // partial slabs per parameter of launch_convblock_bwd (= its grid)
// The attention core of one encoder application (a8 :174-182), every head count and every L: kernels_attn.hip picks the unit of the head size
// (attn.hpp: the contract between those units).  Q / K / V / att / dr / dQ / dK / dV are (R, 128) rows with head h at columns h hd .. h hd + hd - 1,
// mask is the key mask (B, L), lse (B, H, L) is in natural-log units.
struct AttnArgs {
    const float *Q, *K, *V, *mask;
    float *att, *lse;             // forward: outputs (lse may be null: an inference forward does not store it) ; backward: inputs
    const float* dr;              // backward only from here: gradient of r = drop3(att) + x
    float *dQ, *dK, *dV;          // dQ: attn_dq_slabs(L) slabs of (R, 128) that k_qkv_bwd adds
    int B, L, H, b_off;
    Drop d2, d3;                  // probabilities ; attention output (backward only)
};
void launch_attn_fwd(const AttnArgs& a, hipStream_t s);       // L > 128 or H != 8 (8 heads at L <= 128: launch_attn_block_fwd)
// key-major dK / dV for every L.  dQ up to L = ATTN_SLAB_MAX_L (or with VSL_ATTN_DQ_SLABS=1): attn_bwd_dq_slabs(L) partial slabs, one per 256-key
// block; longer: computed query-major, complete in slab 0.  attn_dq_slabs(L) = the slabs written either way (the plan allocates them)
void launch_attn_bwd(const AttnArgs& a, hipStream_t s);
int attn_bwd_dq_slabs(int L);
int attn_dq_slabs(int L);
inline bool attn_heads_supported(int H) { return H == 1 || H == 2 || H == 4 || H == 8 || H == 16; }
// the attention-output block of one encoder application as a launch of its own (a8 :183-190; kernels_head.hip): L > 128 or H != 8
struct AttnOutFwdArgs {
    const float *att, *x;                 // (R,128) attention output ; residual input = the conv block's output
    const float *ln_g, *ln_b, *Wpack, *bo;   // LN2 ; out_layer (forward pack), its bias
    float *r_out, *h2_out, *y_out;        // saved r = drop(att) + x and h2 = drop(LN2(r)) (nullable: an inference forward does not store them) ; block output
    Drop d3, d4, d5;
};
void launch_attn_out_fwd(const AttnOutFwdArgs& a, int R, hipStream_t s);
// attention core + output block of one encoder application in one launch (kernels_enc.hip)
struct AttnBlockArgs {
    const float *Q, *K, *V, *mask, *x;            // q, k, v (R,128) ; key mask (B, L) ; residual input x = conv-block output
    const float *ln_g, *ln_b, *Wpack, *bo;         // LN2, out_layer (forward pack), its bias
    float *att, *lse, *r_out, *h2_out, *y_out;     // saved: att (R,128), LSE (B,H,L), r, h2 ; y = block output
    int L, b_off;
    Drop d2, d3, d4, d5;
    // head_tail (L <= 128 only: attn_block_fwd_hosts_heads): the workgroup goes on with both span heads on its 32 rows (tile_bodies.hpp
    // head_fwd_tile) -- the second predictor pass: hs.feat = the first pass' output (memory), he's features = this kernel's y tile
    int head_tail;
    HeadArgs hs, he;
    const float *head_x, *head_vmask;
    int nosave;                    // inference: att, lse, r_out, h2_out and the heads' hid / lnfeat are not written (may be null; no dropout)
};
void launch_attn_block_fwd(const AttnBlockArgs& a, int B, hipStream_t s);
inline bool attn_block_fwd_hosts_heads(int L) { return L <= 128; }
// the query branch as ONE sample-local launch (kernels_query.hip): Embedding.linear + the whole FeatureEncoder application at L = Lq <= 32,
// one workgroup per sample, 17 KB of LDS.  Saves the same tensors as linear_fwd + convblock_fwd + attn_block_fwd.
struct QueryFwdArgs {
    const float* E;                // (Rq, EW) concatenated word + char embedding rows
    const uint16_t* Wemb3;         // split pack (type 6) of the (128, EW) Embedding.linear weight, K padded to 16
    const float* b_emb;
    float* qf;                     // (Rq,128) Embedding.linear output (nullable)
    const float* pos;              // positional table
    float* x0;
    const uint16_t* W3[4];         // split packs of the pointwise weights
    const uint16_t* Wqkv3;         // split pack of the fused (128, 384) q,k,v operand
    const uint16_t* Wo3;           // split pack of the out_layer weight
    const float *ln_g[4], *ln_b[4], *dw_w[4], *pw_b[4];
    float *y[4], *u[4];
    uint32_t* relu_mask[4];
    Drop dp[4];
    const float *ln1_g, *ln1_b, *bq, *bk, *bv;
    float *h1, *q, *k, *v;
    Drop d1;
    const float* mask;             // (B, L) key mask
    const float *ln2_g, *ln2_b, *bo;
    float *att, *lse, *r, *h2, *out;
    Drop d2, d3, d4, d5;
    int EW, L, b_off;
    int nosave;                    // inference: `out` is the only tensor written (every other output pointer may be null; no dropout)
};
bool query_fused_ok(int L, int H, int EW);         // does the sample-local path take this query length / embedding width?
void launch_query_fwd(const QueryFwdArgs& a, int B, hipStream_t s);
// CQAttention + WeightedPool + CQConcatenate + HighLightLayer + gating (kernels_cq.hip): cq_score, [cq_col,] cq_out read ONE struct, filled once.
struct CqPoolArgs { const float *pool_w, *Wcat, *bcat; float *alpha, *pooled, *pb; };      // a11's WeightedPool and the pooled half of CQConcatenate's Conv1D
bool cq_col_folds(int T, int Lq);
// (nullable -- read by the backward alone, an inference forward does not store them: pool.alpha, pool.pooled, Scol, M, cat, f1, f2)
struct CqFwdArgs {
    const float* C;                       // the context: (B, T, 128), or with vidx a resident (N, T, 128) encoding
    const int* vidx;                      // nullable, device, B ints (vsl_localize / shared step): sample b reads the rows of video vidx[b] (0 <= vidx[b] < N is the
                                          // caller's precondition); every output stays per sample.  nullptr: the instantiations of the training / inference forward
    const float* Qf;                      // (B, Lq, 128) encoded query
    const float *vmask, *qmask;           // (B, T) clip mask, (B, Lq) word mask
    const float *w4C, *w4Q, *w4mlu;       // trilinear weights
    float *S, *Srow, *Scol;               // (B, T, Lq) raw score, row softmax, column softmax
    float *Mpart, *M;                     // [B][ntile][Lq][128] per-tile partials of M = S_col^T C (unfolded column kernel) ; M (B, Lq, 128)
    CqPoolArgs pool;
    const float *Wcqa, *bcqa;             // cqa_linear (forward pack, 4d -> d), its bias
    const float* W1pack;                  // first half of CQConcatenate's (128, 256) weight (forward pack); its pooled half and bias: pool.Wcat / pool.bcat
    const float *wh, *bh;                 // HighLightLayer
    float *cat, *f1, *f2;                 // (R, 512) concat tile, A operand of the cqa_linear weight gradient ; (R,128) CQAttention / CQConcatenate output
    float *hscore, *gated;                // (B, T) ; (R,128) = f2 * hscore
    int B, T, Lq, b_off;
    Drop dc, dq;                          // on C and on Qf in the trilinear score
    int fold;                             // the column kernel folded away (cq_col_folds): k_cq_score gets one extra workgroup per sample for the WeightedPool /
                                          // pooled-bias path, k_cq_out computes the sample's column softmax and M itself from S and launch_cq_col is not called
    const int* qidx = nullptr;            // nullable, device, B ints (vsl_localize_pairs; only together with vidx): Qf is a resident (Q, Lq, 128) encoding and qmask its
                                          // (Q, Lq) mask, sample b reads query qidx[b] (0 <= qidx[b] < Q is the caller's precondition); every output stays per sample
};
void launch_cq_score(const CqFwdArgs& a, hipStream_t s);
void launch_cq_col(const CqFwdArgs& a, hipStream_t s);
void launch_cq_out(const CqFwdArgs& a, hipStream_t s);
// out (B, T) = vmask (N, T) rows vidx[b]: the per-query copy of a resident encoding's clip mask (vsl_localize)
void launch_vmask_gather(const float* vmask, const int* vidx, float* out, int B, int T, hipStream_t s);
void launch_head_fwd(const HeadArgs& a0, const HeadArgs& a1, const float* x, const float* vmask, int R, hipStream_t s);

// ---------------------------------------------------------------- losses / eval
struct LossArgs {
    const float *sl, *el, *h;             // (B, T) start / end logits, highlight score
    const int64_t *s_lab, *e_lab, *h_lab; // (B), (B), (B, T)
    const float* vmask;                   // (B, T)
    int B, T;
    float inv_batch, mask_sum;            // mask_sum > 0: the caller's (global) mask sum ; otherwise the device sums vmask
    float w_loc, w_hl;
    float *scratch, *losses;              // 5 B floats (kernels_head.hip) ; [4]: loc, hl, total, mask_sum
    float *d_sl, *d_el, *d_h;             // gradient seeds (all null: the losses alone)
    unsigned* counter;                    // arrival counter of the one-launch path (nullable: k_loss_a, then k_loss_c or k_loss_b)
};
void launch_loss(const LossArgs& a, hipStream_t s);
void launch_extract_index(const float* sl, const float* el, int64_t* si, int64_t* ei, int B, int T, hipStream_t s);
// top-K spans per sample by greedy selection with temporal NMS (kernels_topk.hip; the semantics: include/vslnet_hip.h, vsl_extract_topk)
struct TopkArgs {
    const float *sl, *el;                 // (B, T) start / end logits
    const int32_t* valid_len;             // (B), nullable = T; clamped into [1, T]
    int B, T, K;                          // 1 <= K <= 32, T <= MAX_L
    float nms_iou;                        // in [0, 1]; 1 suppresses nothing
    int max_span;                         // 0 = unlimited
    int64_t *start_index, *end_index;     // (B, K)
    float *score, *prob;                  // (B, K); prob nullable
    int32_t* count;                       // (B), nullable
};
constexpr int TOPK_MAX_K = 32;
void launch_extract_topk(const TopkArgs& a, hipStream_t s);
// the K_out best candidates of every group of top-K lists (kernels_merge.hip; the semantics: include/vslnet_hip.h, vsl_merge_topk)
struct MergeArgs {
    const int64_t *start, *end;           // (B, K) candidate lists
    const float *score, *key;             // (B, K); the order is by key
    const int32_t* count;                 // (B): filled slots of list b
    const int32_t* group_index;           // (B): group of list b; outside [0, G): none
    const int32_t* tag;                   // (B), or (B, K) with tag_per_slot; nullable = b
    int B, K, G, K_out;                   // 1 <= K, K_out <= 32
    int tag_per_slot;
    int rescan_all;                       // measuring switch: no cached per-thread head
    int32_t *out_tag, *out_list;          // (G, K_out)
    int64_t *out_start, *out_end;
    float *out_score, *out_key;
    int32_t* out_count;                   // (G)
};
void launch_merge_topk(const MergeArgs& a, hipStream_t s);
// the K_out best moments of every group of WINDOW lists in the video's own coordinates, with NMS across the lists (kernels_merge_windows.hip; the
// semantics: include/vslnet_hip.h, vsl_merge_windows)
struct MergeWindowsArgs {
    const int64_t *start, *end;           // (B, K) candidate lists, window-local
    const float *score, *key;             // (B, K); the order is by key
    const int32_t* count;                 // (B): filled slots of list b
    const int32_t* group_index;           // (B): group of list b; outside [0, G): none
    const int32_t* offset;                // (B), nullable = 0: clip index of the list's window start
    int B, K, G, K_out;                   // 1 <= K, K_out <= 32
    float nms_iou;                        // in [0, 1]; identical global spans are suppressed at every value
    int rescan_all;                       // measuring switch: no cached per-thread head
    int32_t* out_list;                    // (G, K_out)
    int64_t *out_start, *out_end;         // global
    float *out_score, *out_key;
    int32_t* out_count;                   // (G)
};
void launch_merge_windows(const MergeWindowsArgs& a, hipStream_t s);
// one relevance score per pair from its highlight scores (kernels_rank.hip; the semantics: include/vslnet_hip.h, vsl_highlight_pairs)
struct RelevanceArgs {
    const float* hscore;                  // (B, T) highlight scores
    const float* vmask;                   // (B, T) the gathered per-pair clip mask the CQ kernels read
    const int *vidx, *qidx;               // (B), device: video / query of pair b (read only when ld > 0)
    float* out;                           // ld > 0: out[qidx[b] * ld + vidx[b]] ; ld == 0: out[b]
    int B, T, ld;
    int mean;                             // 0: max over the valid clips ; 1: their mean.  No valid clip: -inf
};
void launch_pair_relevance(const RelevanceArgs& a, hipStream_t s);
// the best M of N per group (kernels_rank.hip; the semantics: include/vslnet_hip.h, vsl_select_topm)
constexpr int TOPM_MAX_M = 1024;
struct SelectArgs {
    const float* key;                     // (G, N), row stride ld >= N
    int G, N, ld, M;                      // 1 <= M <= TOPM_MAX_M
    int32_t* out_index;                   // (G, M)
    float* out_key;                       // (G, M)
    int32_t* out_count;                   // (G) = min(M, N)
};
void launch_select_topm(const SelectArgs& a, hipStream_t s);
// the grouped training loss: vsl_loss's terms over B pair rows in G groups + a softmax ranking term over every group's relevances
// (kernels_group_loss.hip; the semantics: include/vslnet_hip.h, vsl_group_loss).  Two launches: _a (one workgroup per row: the partials), _c (the seeds;
// block (0, 0): the loss values and the hits)
struct GroupLossArgs {
    const float *sl, *el, *h;             // (B, T) start / end logits, highlight score
    const int64_t *s_lab, *e_lab, *h_lab; // (B), (B), (B, T); s_lab / e_lab nullable together (no span loss), h_lab nullable (no highlight loss)
    const float* vmask;                   // (B, T)
    const int32_t *group_start, *positive;// (G + 1), (G), device
    int B, T, G;
    float inv_pos, inv_groups, mask_sum;  // mask_sum > 0: the caller's (global) mask sum ; otherwise the device sums vmask
    float w_loc, w_hl, w_rank, inv_t;
    int mean;                             // the relevance: 0 max, 1 mean (RelevanceArgs.mean)
    float *scratch, *losses;              // group_loss_scratch_floats(B, G) floats (kernels_group_loss.hip) ; [5]: loc, hl, rank, total, mask_sum
    int32_t* hits;                        // nullable
    float* pair_relevance;                // (B), nullable
    float *d_sl, *d_el, *d_h;             // gradient seeds (all null: the losses alone)
};
inline int64_t group_loss_scratch_floats(int B, int G) { (void)G; return 10 * (int64_t)B + 8; }     // (ten per-row arrays; G: none today)
void launch_group_loss_a(const GroupLossArgs& a, hipStream_t s);
void launch_group_loss_c(const GroupLossArgs& a, hipStream_t s);
// windows over projected feature rows (kernels_window.hip; vsl_encode_windows): out (N, T, 128) = proj rows window_row[n] + t for t < window_len[n]
// inside [0, rows), the projection of a zero feature row (0 + bias) elsewhere ; mask (N, T) = t < window_len[n]
struct WindowGatherArgs {
    const float* proj;                    // (rows, 128) VisualProjection's output over the feature rows
    const float* bias;                    // (128) VisualProjection's bias
    const int32_t *window_row, *window_len;   // (N), device
    float* out;                           // (N, T, 128)
    float* mask;                          // (N, T)
    int N, T, rows;
};
void launch_window_gather(const WindowGatherArgs& a, hipStream_t s);

// ---------------------------------------------------------------- backward
// fuse != nullptr: the end head's workgroups continue with that attention-output backward on their own tile of dfeat (which is then NOT stored)
void launch_head_bwd(const HeadBwdArgs& a0, const HeadBwdArgs& a1, int R, hipStream_t s, const AttnOutBwdArgs* fuse = nullptr);
// a15 DynamicRNN (layers_t7.py:302-313): recurrent part of nn.LSTM(128, 128); the input projection x W_ih^T is a plain GEMM
// (kernels_lstm.hip: one-sample workgroups for B <= 256, which read k_pack's register-order images of W_hh -- PackJob types 9 / 10 -- and
// save tanh(c_t) in tseq; 4-sample MFMA groups beyond, which read W_hh itself).  gates == nullptr (inference): the gates and tseq are not stored, and of
// cseq / hprev the one-sample kernel writes only the rows the next time chunk resumes from
void launch_lstm_fwd(const float* gi, const float* Whh, const float* Wimg, const float* bih, const float* bhh, const float* mask, float* gates,
                     float* cseq, float* tseq, float* hprev, float* out, int B, int T, hipStream_t s, int t0 = 0, int t1 = -1);   // steps [t0, t1)
void launch_lstm_bwd(const float* dout, const float* dout2, const float* mask, const float* gates, const float* cseq, const float* tseq,
                     const float* Whh, const float* Wimg, float* dG, int B, int T, hipStream_t s, float* carry = nullptr, int t0 = 0, int t1 = -1);
                     // steps [t0, t1) in reverse; carry (B, 2, 128): dc / dh handed from one time chunk to the next
constexpr int LSTM_IMG_FLOATS = 4 * D * D;
// The rnn head as one launch per direction: three workgroups per sample (start LSTM, W_ih projection, end LSTM) handing steps over through
// {tag, value} granules.  B <= RNN_FUSED_MAX_B keeps all 3 B workgroups resident beside the side streams' kernels; beyond it the chunked
// launches above.  `epoch` is new for every launch (a NaN-patterned 21-bit counter); forward.hip clears a plan's granule buffers once per
// workspace and once more whenever the counter has wrapped (rnn_granules_fresh), so a stale word never carries the live tag.
constexpr int RNN_FUSED_MAX_B = 80;
struct RnnFwdArgs {
    const float* gi0;                 // (R, 512) input projection of the start LSTM
    const float* Whh[2];              // PackJob type 9 images of W_hh
    const float* Wih1;                // PackJob type 9 image of the end LSTM's W_ih
    const float* bih[2]; const float* bhh[2];
    const float* mask;
    float* gates[2]; float* cseq[2]; float* tseq[2]; float* hprev[2]; float* out[2];
    unsigned long long* h_gran;       // (R, 128) start LSTM's h * mask
    unsigned long long* gi_gran;      // (R, 512) W_ih1 (h * mask)
    unsigned epoch;
    int B, T;
    int nosave;                       // inference: `out` is the only sequence written (gates, cseq, tseq, hprev may be null)
};
struct RnnBwdArgs {
    const float* dout[2];             // (R, 128) gradients wrt the LSTM outputs coming from the span heads
    const float* mask;
    const float* gates[2]; const float* cseq[2]; const float* tseq[2];
    const float* Whh[2];              // PackJob type 10 images of W_hh
    const float* Wih1;                // PackJob type 10 image of the end LSTM's W_ih
    float* dG[2];
    unsigned long long* dg_gran;      // (R, 512) end LSTM's gate gradients
    unsigned long long* dx_gran;      // (R, 128) dG W_ih1: the start LSTM's second incoming gradient
    unsigned epoch;
    int B, T;
};
bool rnn_fused_ok(int B);
void launch_rnn_fwd(const RnnFwdArgs& a, hipStream_t s);
void launch_rnn_bwd(const RnnBwdArgs& a, hipStream_t s);      // one image = W_hh in the register order of k_lstm1_fwd (type 9) / k_lstm1_bwd (type 10)
void launch_wgrad(const WgradBatch& wb, hipStream_t s);     // kernels_wgrad.hip
void launch_attn_out_bwd(const AttnOutBwdArgs& a, int R, hipStream_t s);
void launch_qkv_bwd(const float* dQ, const float* dK, const float* dV, const float* x, const float* dr,
                    const float* ln_g, const uint16_t* WT3 /* split pack of the (384, 128) operand */, float* dx, float* p_lng, float* p_lnb, int R,
                    Drop d1, hipStream_t s, int dq_slabs = 1);
void launch_cqcat_bwd(const CqcatBwdArgs& a, int R, hipStream_t s);
struct CqBwdArgs {
    const float *df1, *df2, *C, *Qf, *Srow, *Scol, *M, *alpha, *pooled;      // saved forward tensors / incoming grads
    const float *WcqaT;                                                        // transpose pack of cqa_linear (ncols 512)
    const float *w4C, *w4Q, *w4mlu, *pool_w, *Wcat;
    float *dC;            // (B,T,128) out: total grad wrt the video encoder output
    float *dQ;            // (B,Lq,128) out: total grad wrt the query encoder output
    float *dSr, *dSs;     // (B,T,Lq) scratch: row-softmax backward, dS_col
    float *P1;            // [B][ntile][2][Lq][128] per-tile partials of dM and dQ(c2q)
    float *P2, *P3;       // [B][ntile][Lq] partials of the column-softmax dot / colsum(dS)
    float *P4;            // [B][ntile][Lq][128] partial of dQ(trilinear)
    float *P5;            // [B][ntile][128] partial of colsum(df2)
    float *p_w4C, *p_w4mlu;                              // parameter slabs [B * ntile][128]
    float *p_w4Q, *p_pool, *p_bcat;                      // parameter slabs [B][128]
    float *p_W2;                                         // [B][128][128] for Wcat[:, 128:]
    int T, Lq, b_off, ntile;
    Drop dc, dq;
    const int* vidx;      // nullable (B), device: C is the (N, T, 128) encoding of a shared-video training step and sample b reads video vidx[b]; everything written stays at sample b
};
void launch_cq_bwd(const CqBwdArgs& a, int B, hipStream_t s);          // kernels a, b, c: dC final, dQ partials
void launch_cq_bwd_query(const CqBwdArgs& a, int B, hipStream_t s);    // kernel d: dQ + pooled-query parameters
// training through a shared video encoding (kernels_shared.hip): the CSR of the queries of each video (start[N + 1], members[B] ascending within a
// video) from the device index, and dCv (N, T, 128) = the sum of dC (B, T, 128) over each video's queries in member order
void launch_group_csr(const int* vidx, int B, int N, int* start, int* members, hipStream_t s);
void launch_group_sum(const float* dC, const int* start, const int* members, float* dCv, int N, int T, hipStream_t s);
// the backward of that launch (autograd of the same lines) + the Embedding linear's data gradient; per-SAMPLE partial slabs
struct QueryBwdArgs {
    const float* dout;             // (Rq,128) grad wrt the encoder output
    const float *r, *ln2_g;        // output block
    const uint16_t* WoT3;          // split pack (type 7) of the out_layer weight
    float *go, *p_ln2g, *p_ln2b;
    Drop d2, d3, d4, d5;
    const float *q, *k, *v, *att, *lse, *mask;     // attention
    float *dq, *dk, *dv;
    const uint16_t* WqkvT3;        // split pack (type 7) of [Wq; Wk; Wv]: 384 contraction rows
    const float *y3, *ln1_g;
    float *p_ln1g, *p_ln1b;
    Drop d1;
    const uint16_t* WT3[4];        // conv layers
    const float* x[4];
    const uint32_t* relu_mask[4];
    const float *ln_g[4], *ln_b[4], *dw_w[4];
    Drop dp[4];
    float* gz[4];
    float *p_lng[4], *p_lnb[4], *p_dw[4];
    float* dx0;
    const uint16_t* WembT3;        // split pack (type 7) of the Embedding.linear weight, EWc >= EW columns
    float* dE;
    int EW, EWc, L, b_off;
};
void launch_query_bwd(const QueryBwdArgs& a, int B, hipStream_t s);
struct EmbedBwdArgs {
    const float* dE;                      // (Rq, word_dim + 100) grad wrt the concatenated embedding rows
    const int64_t *word_ids, *char_ids;
    const float* E;                       // forward output (relu mask of the char channels)
    const int8_t* argpos;                 // (Rq, 100) saved arg-max positions
    const float *char_tab, *wimg_b;       // wimg_b: char-conv B-operand image (PackJob type 8)
    float *p_cw, *p_cb;                   // partial slabs [nchunk][300 char_dim], [nchunk][100]
    float *p_tab, *p_unk;                 // [nchunk][char_size * char_dim], [nchunk][word_dim] (p_unk nullable: trainable word table -> launch_word_table_bwd)
    int Rq, Lc, word_dim, char_dim, char_size;
    Drop dw, dc;
};
void launch_embed_bwd(const EmbedBwdArgs& a, hipStream_t s);
void launch_word_table_bwd(const float* dE, const int64_t* word_ids, float* gtab /*(word_size, word_dim) inside the gradient bucket*/, int Rq,
                           int word_size, int word_dim, Drop dw, bool accumulate /* add to the rows the batch touches, leave the others */, hipStream_t s);
// VisualProjection's data gradient (kernels_vproj_dx.hip; vsl_input_grads): dX (R, Dv) = m * (G W), m = the forward's dropout multiplier of each feature
struct VprojDxArgs {
    const float* G;                       // (R, 128) grad wrt VisualProjection's output (the plan's dvf)
    const float* W;                       // (128, Dv) the Conv1D weight, unpacked, in the parameter bucket
    float* dX;                            // (R, Dv) out
    int R, Dv;                            // Dv: a multiple of 4, any size
    Drop dp;                              // the forward's SITE_VIS
    int cus;                              // CUs of the device (0: unknown): sizes the grid's second dimension
};
void launch_vproj_dx(const VprojDxArgs& a, hipStream_t s);
void launch_reduce(const float* partial, float* grads, const ReduceSeg* segs_dev, const int* blk2seg_dev, int nblocks,
                   float* sq /* [nblocks]: sum of squares of each block's results */, bool accumulate /* grads += the sums ; sq of the stored values */,
                   hipStream_t s);
// fused optimizer (vsl_adamw_step): sum of squares partials, then clip + AdamW
constexpr int OPT_BLOCKS = 256;
struct AdamHp { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; int hf_order; };      // bc1 = 1 - b1^step ; bc2_sqrt = sqrt(1 - b2^step)
struct AdamwArgs {
    float* params; const float* grads; float *m, *v;
    const uint8_t* decay_mask;
    float* partials;                      // [OPT_BLOCKS + 1] scratch of the k_sqsum pass
    int64_t n;
    float clip;                           // clip_grad_norm_ bound (<= 0: none)
    AdamHp hp;
    float* norm_out;                      // nullable
    const float* sq_from_backward; int nsq;   // k_reduce's nsq partials instead of a k_sqsum pass (nullable)
};
void launch_adamw(const AdamwArgs& a, hipStream_t s);
constexpr int EMB_CHUNK_MAX = 8;  // most query words per workgroup in the embedding backward
int embed_bwd_chunk(int Rq, int Lc, int char_dim);      // words per workgroup the launcher uses (the number of partial slabs follows from it)
constexpr int EB_IMG_Q = 76;      // k-steps of the embedding backward's B-operand image ([channel tile][76][64 lanes], PackJob type 8)

// A switch of the environment: VSL_X=0 turns off what is on by default, VSL_X=1 turns on what is off, anything else leaves the default.  A call
// site keeps the answer in a function-local static, so that a process reads each switch once.
inline bool switch_on(const char* name, bool dflt) { const char* e = getenv(name); return e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : dflt; }

}  // namespace vsl
