/* libvslnet_hip.so -- C ABI of the MI355X-native VSLNet forward/backward path.
 *
 * The reference (26hzhang/VSLNet) has no FFI / plugin interface: the hot path sits behind an ordinary Python class
 * (`model/VSLNet_t7.py:20-72`).  This ABI is therefore NEW; it is shaped so that the reference-side binding is one
 * thin `nn.Module` (vslnet_amd/model/VSLNet.py, loaded with ctypes -- see INTEGRATION.md).  Each entry point names the
 * reference interface it replaces.
 *
 * Conventions
 *   - plain C: opaque handle, plain pointers and sizes, no torch / C++ types in any signature;
 *   - every pointer inside `vsl_io` is a DEVICE pointer into caller-owned memory (PyTorch-ROCm tensors are used for
 *     storage only); the library owns nothing but the handle and its small per-shape plans;
 *   - all work is enqueued asynchronously on the caller's `hipStream_t` (passed as void*);
 *   - return value 0 = ok, non-zero = error; `vsl_last_error()` returns a thread-local message; nothing throws
 *     across the ABI;  one handle per device, not thread-safe per handle.
 *   - fp32 everywhere (the reference is IEEE fp32 end to end), ids/labels int64, masks fp32 0/1.
 */
#ifndef VSLNET_HIP_H
#define VSLNET_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vsl_handle_s* vsl_handle;

/* fields of the `configs` namespace read by VSLNet.__init__ (VSLNet_t7.py:24-38) */
typedef struct {
    int32_t dim;               /* configs.dim              (kernels are specialised for 128)              */
    int32_t num_heads;         /* configs.num_heads (1, 2, 4, 8 or 16: head size 128, 64, 32, 16 or 8)    */
    int32_t max_pos_len;       /* configs.max_pos_len      (rows of the positional table; T, Lq <= it)    */
    int32_t video_feature_dim; /* configs.video_feature_dim (multiple of 4: 1024 I3D, 4096 / 500 C3D)         */
    int32_t word_dim;          /* configs.word_dim = 300   (word_dim + 100 must be a multiple of 8)       */
    int32_t char_dim;          /* configs.char_dim = 50    (<= 128)                                       */
    int32_t word_size;         /* configs.word_size  = rows of [pad; unk; glove]                          */
    int32_t char_size;         /* configs.char_size  = rows of the character table                        */
    int32_t predictor;         /* 0 = 'rnn' (DynamicRNN, layers_t7.py:302-313), 1 = 'transformer'         */
    float drop_rate;           /* configs.drop_rate                                                        */
    int32_t word_table;        /* 0: WordEmbedding(word_vectors=GloVe): frozen [pad; glove] + trainable unk_vec (layers_t7.py:29-34)
                                * 1: WordEmbedding(word_vectors=None): trainable nn.Embedding(word_size, word_dim, padding_idx=0)
                                *    (:36) -- the parameter "embedding_net.word_emb.word_emb.weight" replaces unk_vec and
                                *    vsl_io.pad_vec / glove_vec are ignored (may be NULL)                                  */
} vsl_config;

/* One forward / backward problem instance.  Replaces the argument list of VSLNet.forward (VSLNet_t7.py:52) plus
 * the tensors autograd keeps alive between forward and `total_loss.backward()` (main_t7.py:103-110). */
typedef struct {
    int32_t B, T, Lq, Lc;          /* batch, padded clips (T <= 4096), padded query words, padded chars per word  */
    /* parameters */
    const float* params;           /* flat trainable parameter bucket, layout = vsl_param_info()                   */
    const float* pad_vec;          /* embedding_net.word_emb.pad_vec   (1, word_dim)  frozen                       */
    const float* glove_vec;        /* embedding_net.word_emb.glove_vec (word_size-2, word_dim) frozen              */
    /* batch (VSLNet_t7.py:52) */
    const int64_t* word_ids;       /* (B, Lq)                                                                      */
    const int64_t* char_ids;       /* (B, Lq, Lc)                                                                  */
    const float* video_features;   /* (B, T, video_feature_dim)                                                    */
    const float* v_mask;           /* (B, T)                                                                       */
    const float* q_mask;           /* (B, Lq)                                                                      */
    /* outputs (VSLNet_t7.py:62) */
    float* h_score;                /* (B, T)  exactly 0 at padded clips                                            */
    float* start_logits;           /* (B, T)  exactly -1e30 at padded clips                                        */
    float* end_logits;             /* (B, T)                                                                       */
    /* saved activations + backward temporaries; vsl_workspace_floats() floats, caller-owned, 16-byte aligned.      */
    /* Needs no initialisation, may be reused between shapes and handles.  The rnn head's in-launch hand-off buffers */
    /* live here: their tags are per-process NaN-patterned epochs (a 21-bit counter); the library clears a plan's   */
    /* hand-off range once per workspace pointer and again whenever the counter has wrapped.  A caller that writes  */
    /* its own data into a workspace between two steps of the SAME shape must hand over a different pointer (or     */
    /* re-create the handle): inside one generation a word of that range is assumed to be the library's own.        */
    float* workspace;
    /* dropout (nn.Dropout sites of layers_t7.py): counter-based masks, keyed by (seed, site, element)             */
    int32_t training;              /* 0: eval (no dropout)                                                         */
    uint64_t seed;                 /* change every step; the backward must see the forward's value                 */
    /* backward inputs / outputs */
    const float* d_h_score;        /* (B, T) dLoss/dh_score      (nullable = zeros)                                */
    const float* d_start_logits;   /* (B, T)                                                                        */
    const float* d_end_logits;     /* (B, T)                                                                        */
    float* grads;                  /* flat gradient bucket, same layout as `params` (overwritten; vsl_backward_accumulate adds) */
    /* data parallel: index of this shard's first sample in the GLOBAL batch.  The dropout element counters continue
     * from it, so for one seed the masks -- and with the global loss normalisers the summed gradient -- do not depend
     * on how many ranks the batch is split over (shards keep the global padded T / Lq / Lc).  0 = single process.  */
    int32_t sample_offset;
    /* bf16 THROUGHPUT mode (BASELINE configs[1] says "bf16"; the reference itself is fp32 end to end, so this is a separate mode
     * with its own tolerance, never the parity path): when non-NULL, the (B, T, video_feature_dim) features are read from this
     * bfloat16 copy instead of `video_features` (which may then be NULL) -- half the bytes of the only large HBM stream -- and
     * VisualProjection runs on the bf16 matrix cores (bf16 features x bf16-rounded weight, fp32 accumulate; the dropout scale is
     * applied to the fp32 sum).  Its weight gradient reads the same bf16 features (fp32 MFMA).  Everything else stays fp32. */
    const uint16_t* video_features_bf16;
    /* data parallel, optional (NULL = off): a caller-owned hipEvent_t that vsl_backward records as soon as the gradients of the
     * parameters at float offsets >= vsl_early_grad_offset() are FINAL in `grads` (the predictor block: about 55 % into the backward).
     * The caller can start their all-reduce on another stream behind this event while the rest of the backward runs; the remaining
     * offsets are final when vsl_backward's work on the caller's stream completes.  No reference counterpart (main_t7.py has no
     * distributed code); it is what makes the ONE exchange of SURVEY 8(e) overlap with the backward. */
    void* early_grads_event;
    /* single process, optional (NULL = off): the optimizer step of main_t7.py:111-113 applied by vsl_backward itself, behind its final
     * reduction (see vsl_fused_step below).  Not for data-parallel callers: their gradients are exchanged between the backward and the update. */
    const struct vsl_fused_step* fused_step;
    /* optional (NULL = off): vsl_loss folded into vsl_backward -- the call first does what vsl_loss(h, io, fused_loss) does (losses and the three
     * seeds are written exactly as vsl_loss writes them; complete when vsl_backward's work on the caller's stream is), then runs the backward
     * from those seeds; vsl_io.d_h_score / d_start_logits / d_end_logits are ignored.  For T >= 32 with the caller's mask_sum
     * the loss launch leaves the dependent chain: the span heads' and the highlight layer's backward compute their seeds from the logits
     * themselves (VSLNet_t7.py:67-72 and main_t7.py:107-110 as one call). */
    const struct vsl_loss_io* fused_loss;
    /* INFERENCE mode (0 = off: everything above): a forward that will never be differentiated.  The forward kernels store only what a later
     * forward kernel reads (no saved activation, no ReLU words, no LSE), and `workspace` needs vsl_inference_workspace_floats() floats only:
     * a forward-only plan whose buffers are reused by liveness.  The outputs are bit for bit those of vsl_forward with training = 0.
     * Excludes `training` (there is no dropout in this mode).  vsl_backward on this io, or in this workspace before another training forward
     * has run in it, is an error, and so is vsl_workspace_offset: there is nothing saved.  vsl_loss and the launch ledger work.
     * This is evaluation under torch.no_grad() (runner.eval_test, main.py --mode test); the reference has no counterpart. */
    int32_t inference;
} vsl_io;
/* Every struct of this header must be zero-initialised by the caller before the fields are set: new optional fields are appended, and
 * zero means "off".  vsl_abi_version() changes whenever a struct layout or an entry point's meaning changes; a binding checks it once. */
#define VSL_ABI_VERSION 9
int vsl_abi_version(void);

/* labels + weights for the fused loss (replaces compute_loss / compute_highlight_loss, VSLNet_t7.py:67-72, and the
 * combination `loc + highlight_lambda * hl` of main_t7.py:107).  Data-parallel callers pass the GLOBAL normalisers. */
typedef struct vsl_loss_io {
    const int64_t* start_labels;   /* (B)    */
    const int64_t* end_labels;     /* (B)    */
    const int64_t* h_labels;       /* (B, T) */
    float w_loc;                   /* weight of CE(start)+CE(end)      (main_t7.py: 1.0)                           */
    float w_highlight;             /* weight of the highlight loss     (main_t7.py: highlight_lambda = 5.0)        */
    float inv_batch;               /* 1 / global batch size (CrossEntropyLoss(mean), layers_t7.py:367-368)         */
    float mask_sum;                /* global sum(v_mask) (layers_t7.py:298); <= 0: use this batch's own sum        */
    float* losses;                 /* out, device, 4 floats: loc, highlight, w_loc*loc + w_hl*hl, mask_sum used     */
    float* d_h_score;              /* out (B, T), nullable: seeds for vsl_backward                                  */
    float* d_start_logits;         /* out (B, T)                                                                    */
    float* d_end_logits;           /* out (B, T)                                                                    */
} vsl_loss_io;

const char* vsl_last_error(void);

/* VSLNet.__init__ (VSLNet_t7.py:21-40): validates the config, fixes the flat parameter layout. */
int vsl_create(const vsl_config* cfg, vsl_handle* out);
int vsl_destroy(vsl_handle h);

/* flat parameter bucket layout; names and shapes are the reference's state_dict entries, trainable only
 * (pad_vec / glove_vec are passed separately in vsl_io). */
int vsl_param_count(vsl_handle h);
int vsl_param_info(vsl_handle h, int index, char* name, int name_cap, int64_t* offset, int64_t* numel, int32_t* ndim,
                   int64_t dims[4]);
int64_t vsl_param_floats(vsl_handle h);

/* number of floats the caller must provide in vsl_io.workspace for this shape (the training plan: every saved activation, the backward's
 * temporaries and partial slabs; also enough for an inference forward of the same shape) */
int vsl_workspace_floats(vsl_handle h, int B, int T, int Lq, int Lc, int64_t* out);
/* the same for a forward with vsl_io.inference != 0: the forward-only plan (a handful of live (B T, 128) tensors; never more than
 * vsl_workspace_floats() of the shape).  A shape whose training plan exceeds the 2^31-float limit may still fit this one.  No reference counterpart. */
int vsl_inference_workspace_floats(vsl_handle h, int B, int T, int Lq, int Lc, int64_t* out);

/* VSLNet.forward (VSLNet_t7.py:52-62) */
int vsl_forward(vsl_handle h, const vsl_io* io, void* hip_stream);

/* ONE ENCODING PER VIDEO, MANY QUERIES AGAINST IT (evaluation only: no dropout, nothing saved, no backward; the reference has no counterpart -- it
 * encodes the video once per query).  VisualProjection and the video pass of the shared feature encoder do not depend on the query, and nothing
 * behind them reads the raw features: vsl_encode_video runs that half for N videos, vsl_localize runs everything else for B queries, query b against
 * video video_index[b] of the encoding.  Together they give what vsl_forward (inference = 1) gives on the replicated batch
 * video_features[video_index], v_mask[video_index]: bit for bit when T is a multiple of 32 or at most 32; at other T within a few 1e-6, because the conv-block
 * kernel of such T rounds a row differently depending on where its sample sits in the batch -- two vsl_forward calls that hold the
 * same video at different batch positions differ in the same way.
 * AN ENCODING BELONGS TO ITS PADDED T (and to the parameter values it was computed with): the conv block's zero padding at the sequence end turns into
 * pad-row values when T grows and the attention spreads them to every row, so the same video encoded at another T differs on its valid rows too.  One T
 * serves the encoding, the mask and the logits; a caller re-encodes after the parameters change.
 * Both calls mark their workspace like an inference forward: vsl_backward in it, and vsl_workspace_offset, are errors until a training forward has run.
 * The addressing limits of vsl_forward (2^31 workspace floats, N T 128 resp. B T 128 floats below 2 GiB) apply to N here and to B there.
 * Detect the feature by the presence of the symbols: VSL_ABI_VERSION does not change for an added entry point. */
typedef struct {                       /* zero-initialise; new fields are appended */
    int32_t N, T;                      /* videos (>= 1), padded clips (T <= 4096)                                                          */
    const float* params;               /* flat parameter bucket                                                                            */
    const float* video_features;       /* (N, T, video_feature_dim), or NULL with the bf16 copy                                            */
    const uint16_t* video_features_bf16; /* bf16 throughput mode, as vsl_io.video_features_bf16                                            */
    const float* v_mask;               /* (N, T)                                                                                           */
    float* video_encoding;             /* out (N, T, 128): the shared feature encoder's output on the projected features                   */
    float* workspace;                  /* vsl_encode_workspace_floats() floats: the operand packs and one encoder application's scratch    */
} vsl_encode_io;
int vsl_encode_workspace_floats(vsl_handle h, int N, int T, int64_t* out);
int vsl_encode_video(vsl_handle h, const vsl_encode_io* io, void* hip_stream);

typedef struct {                       /* zero-initialise; new fields are appended */
    int32_t B, T, Lq, Lc, N;           /* queries; T of the encoding; padded query words / chars per word; videos in the encoding          */
    const float* params;               /* the SAME parameter values the encoding was computed with                                         */
    const float* pad_vec;              /* as in vsl_io                                                                                     */
    const float* glove_vec;
    const int64_t* word_ids;           /* (B, Lq)                                                                                          */
    const int64_t* char_ids;           /* (B, Lq, Lc)                                                                                      */
    const float* q_mask;               /* (B, Lq)                                                                                          */
    const float* video_encoding;       /* (N, T, 128) from vsl_encode_video with the SAME T                                                */
    const float* v_mask;               /* (N, T): per VIDEO                                                                                */
    const int32_t* video_index;        /* (B), device: video of query b.  0 <= value < N is the CALLER'S precondition: the library does not */
                                       /* read it on the host, and an index outside the range reads outside the encoding                   */
    float* h_score;                    /* out (B, T), as vsl_forward writes them                                                           */
    float* start_logits;
    float* end_logits;
    float* workspace;                  /* vsl_localize_workspace_floats() floats: the inference plan of (B, T, Lq, Lc) without a video pass  */
                                       /* plus the (B, T) gathered mask; it never holds a (B, T, 128) copy of the encoding                 */
} vsl_localize_io;
int vsl_localize_workspace_floats(vsl_handle h, int B, int T, int Lq, int Lc, int64_t* out);
int vsl_localize(vsl_handle h, const vsl_localize_io* io, void* hip_stream);

/* ONE ENCODING PER QUERY, TO BE ASKED ABOUT MANY VIDEOS (evaluation only: no dropout, nothing saved, no backward; no reference counterpart).  The word +
 * char embedding, the Embedding linear and the query pass of the shared feature encoder do not depend on the video: vsl_encode_query runs that half of
 * the inference forward for Q queries and writes the encoder's output -- bit for bit what vsl_forward's query branch leaves as the saved activation
 * "qenc" for the same Q queries with training = 0 -- into the caller's (Q, Lq, 128) buffer.  It packs only the operands it reads (the char-conv image,
 * the shared encoder's and the Embedding linear's; not VisualProjection's, the largest) and runs on the caller's stream alone.
 * AN ENCODING BELONGS TO ITS PADDED Lq, to the Lc it was embedded at and to the parameter values it was computed with: the conv block's zero padding
 * at the sequence end turns into pad-row values when Lq grows.  Where the query path is not sample-local (Lq > 32, or num_heads other than 8) a row is
 * also rounded by its query's position in the batch when Lq is no multiple of 32, as vsl_encode_video records for T.  A caller re-encodes after the
 * parameters change.
 * The call marks its workspace like an inference forward: vsl_backward in it, and vsl_workspace_offset, are errors until a training forward has run.
 * The trainable word table (word_table = 1: pad_vec / glove_vec ignored) works as in vsl_forward.  Limits: Q >= 1, 1 <= Lq <= min(max_pos_len, 128),
 * Lc as in vsl_forward, Q Lq 128 floats below 2 GiB.  Detect the feature by the presence of the symbols: VSL_ABI_VERSION does not change for an added
 * entry point. */
typedef struct {                       /* zero-initialise; new fields are appended */
    int32_t Q, Lq, Lc;                 /* queries (>= 1); padded query words / chars per word                                              */
    const float* params;               /* flat parameter bucket                                                                            */
    const float* pad_vec;              /* as in vsl_io                                                                                     */
    const float* glove_vec;
    const int64_t* word_ids;           /* (Q, Lq)                                                                                          */
    const int64_t* char_ids;           /* (Q, Lq, Lc)                                                                                      */
    const float* q_mask;               /* (Q, Lq)                                                                                          */
    float* query_encoding;             /* out (Q, Lq, 128): the shared feature encoder's output on the embedded queries                    */
    float* workspace;                  /* vsl_encode_query_workspace_floats() floats: the operand packs and the query branch's scratch      */
} vsl_encode_query_io;
int vsl_encode_query_workspace_floats(vsl_handle h, int Q, int Lq, int Lc, int64_t* out);
int vsl_encode_query(vsl_handle h, const vsl_encode_query_io* io, void* hip_stream);

/* PAIRS OF RESIDENT ENCODINGS: vsl_localize with no query branch at all (evaluation only; no reference counterpart).  Pair b reads video
 * video_index[b] of an (N, T, 128) encoding from vsl_encode_video and query query_index[b] of a (Q, Lq, 128) encoding from vsl_encode_query with its
 * (Q, Lq) mask; the call runs CQAttention, CQConcatenate, the highlight layer, the predictor and the span heads for the B pairs and writes what
 * vsl_localize writes for the replicated queries word_ids[query_index], char_ids[query_index], q_mask[query_index] -- bit for bit where the query
 * encoding does not depend on the query's position in its batch (num_heads 8 with Lq <= 32, or Lq a multiple of 32), within a few 1e-6 otherwise (see
 * vsl_encode_query).  The reads of both encodings and of the word mask go through the indices (one scalar load per workgroup); everything written
 * stays at pair b, and nothing here ever holds a (B, T, 128) or (B, Lq, 128) copy of an encoding.  It packs only the operands behind the two branches.
 * Both encodings must come from the SAME parameter values as `params`, at this T and this Lq.  The indices are device arrays; 0 <= video_index[b] < N
 * and 0 <= query_index[b] < Q are the CALLER'S precondition: the library does not read them on the host, and an index outside its range reads outside
 * the encoding.  Refused by name: B, N, Q < 1; NULL encodings, masks or indices; Lq > 128; T > 4096 (and the limits of vsl_forward on T, Lq, B T).
 * The call marks its workspace like an inference forward.  Detect the feature by the presence of the symbols: VSL_ABI_VERSION does not change for an
 * added entry point. */
typedef struct {                       /* zero-initialise; new fields are appended */
    int32_t B, T, Lq, N, Q;            /* pairs; T of the video encoding; Lq of the query encoding; videos / queries in the encodings      */
    const float* params;               /* the SAME parameter values both encodings were computed with                                      */
    const float* video_encoding;       /* (N, T, 128) from vsl_encode_video with the SAME T                                                */
    const float* v_mask;               /* (N, T): per VIDEO                                                                                */
    const float* query_encoding;       /* (Q, Lq, 128) from vsl_encode_query with the SAME Lq                                              */
    const float* q_mask;               /* (Q, Lq): per QUERY                                                                               */
    const int32_t* video_index;        /* (B), device: video of pair b                                                                     */
    const int32_t* query_index;        /* (B), device: query of pair b                                                                     */
    float* h_score;                    /* out (B, T), as vsl_forward writes them                                                           */
    float* start_logits;
    float* end_logits;
    float* workspace;                  /* vsl_pairs_workspace_floats() floats: the vsl_localize plan without the query branch's scratch    */
} vsl_pairs_io;
int vsl_pairs_workspace_floats(vsl_handle h, int B, int T, int Lq, int64_t* out);
int vsl_localize_pairs(vsl_handle h, const vsl_pairs_io* io, void* hip_stream);

/* COARSE-TO-FINE CORPUS SEARCH, THE COARSE HALF: which videos are relevant to a query (evaluation only; no reference counterpart).
 *
 * vsl_highlight_pairs: vsl_localize_pairs that stops behind the highlight layer.  It enqueues what vsl_localize_pairs enqueues up to and including the
 * launch that writes h_score -- the operand pack, the mask gather, the CQAttention / CQConcatenate / highlight kernels, the same kernels in the same
 * order -- and neither the predictor nor the span heads.  `pairs` is read as vsl_localize_pairs reads it, except:
 *   - pairs.start_logits / pairs.end_logits are ignored (may be NULL);
 *   - pairs.h_score may be NULL: the (B, T) scores then stay in the workspace.  When given it receives, bit for bit, what vsl_localize_pairs writes
 *     for the same pairs;
 *   - pairs.workspace: vsl_pairs_workspace_floats() floats, the plan of vsl_localize_pairs (its predictor slots are simply not used).
 * Behind it, on the same stream, ONE launch (ledger label "pair_relevance") reduces every pair's h_score row to one float over the pair's VALID clips
 * (the gathered per-pair mask the CQ kernels read):
 *   - relevance = 0: the maximum -- exact;
 *   - relevance = 1: the mean, sum / count in fp32.  The order of the additions is a function of T alone (one wave per pair: lane l adds clips l,
 *     l + 64, ... ascending, a butterfly joins the lanes): the same bits on every run and at every position b of the pair in the call;
 *   - a pair without a valid clip: -INFINITY.
 * Output addressing: ld > 0: out[query_index[b] * ld + video_index[b]] -- a (Q, ld) relevance matrix filled chunk by chunk, no strided copy; two pairs
 * of one call with the same (query, video) write the same value.  ld == 0: out[b].
 * Refused by name: every refusal of vsl_localize_pairs but the two logits pointers; relevance other than 0 or 1; a NULL out; 0 < ld < N.
 * The call marks its workspace like an inference forward.  Detect the feature by the presence of the symbols: VSL_ABI_VERSION does not change for
 * an added entry point. */
typedef struct vsl_highlight_io {          /* zero-initialise; new fields are appended */
    vsl_pairs_io pairs;
    int32_t relevance;                     /* 0 = max, 1 = mean                                                                                */
    int32_t ld;                            /* 0: out is (B) ; >= N: out is a (Q, ld) matrix                                                    */
    float* out;
} vsl_highlight_io;
int vsl_highlight_pairs(vsl_handle h, const vsl_highlight_io* io, void* hip_stream);

/* vsl_select_topm: the best M of N per group on the device.  `key` is (G, N) fp32 with row stride ld >= N (the relevance matrix above: group = query,
 * index = video).  Per group g:
 *   - order: key descending, ties by the SMALLER index; -0.0 counts as +0.0 (keys are compared as key + 0.0f).  A strict total order: the result is a
 *     pure function of the input, the same bits on every run; no atomic on global memory, none on a float;
 *   - out_count[g] = min(M, N); out_index[g][r], out_key[g][r] (the key as compared: key + 0.0f) for r < count are the first `count` indices IN THAT
 *     ORDER, ranked; slots from count on hold -1 and 0.
 * M >= N sorts the whole row (N <= 1024).  A NaN key gives an unspecified choice (every loop is bounded by N and M).
 * Limits, each refused by name: 1 <= M <= 1024; G, N >= 1; ld >= N; G * ld < 2^31; NULL pointers.  A free-standing call like vsl_merge_topk: no plan, no
 * workspace; one workgroup per group, ONE launch on the caller's stream.  Detect the feature by the presence of the symbol. */
typedef struct vsl_select_io {             /* zero-initialise; new fields are appended */
    int32_t G, N, ld, M;
    const float* key;                      /* (G, N), row stride ld                                                                            */
    int32_t* out_index;                    /* (G, M)                                                                                           */
    float* out_key;                        /* (G, M)                                                                                           */
    int32_t* out_count;                    /* (G)                                                                                              */
} vsl_select_io;
int vsl_select_topm(vsl_handle h, const vsl_select_io* io, void* hip_stream);

/* TRAINING THROUGH A SHARED VIDEO ENCODING: one step over N videos and B queries, query b paired with video video_index[b] (no reference counterpart:
 * it runs the video half once per sample).  VisualProjection and encoder application 0 run forward AND backward on N T rows; the query branch,
 * CQAttention, CQConcatenate, the highlight layer, the predictor, the span heads and the losses run on B samples as in vsl_forward / vsl_backward.
 * In these calls the vsl_io fields carry: video_features (or the bf16 copy) as (N, T, video_feature_dim); v_mask as the (B, T) PER-QUERY mask, i.e.
 * video_v_mask[video_index] (vsl_loss then works unchanged); outputs and seeds as (B, T); training = 1, or 0 for the saved evaluation path.
 * Semantics:
 *   - dropout: the sites of the video half -- VisualProjection's input and sites 0..8 of encoder application 0 -- are keyed by the element index in
 *     their (N, T, .) tensors: ONE mask per video, shared by its queries.  Every other site keeps its (B, .) keying, CQAttention's context dropout
 *     included (it applies to sample b).  At drop_rate 0 the step is mathematically vsl_forward / vsl_backward on the replicated batch
 *     video_features[video_index]; at drop_rate > 0 it is a different but equally valid stochastic estimate -- not reference parity;
 *   - the gradient of the encoding is dCv[n] = sum over {b : video_index[b] = n} of dC[b], added in ASCENDING b.  There is no floating-point atomic
 *     anywhere in the path: two runs of the same step give bit-identical gradients.  A video without a query gets a zero dCv and contributes nothing;
 *   - the encoding is computed inside the step at the batch's T, so the rule of vsl_encode_video about an encoding and its padded T does not arise.
 * vsl_io.inference != 0 is refused (use vsl_encode_video + vsl_localize), and so are a non-zero sample_offset and early_grads_event (data parallel is not
 * supported through a shared encoding).  fused_loss and fused_step work as in vsl_backward.  The handle remembers what its last forward was:
 * vsl_backward after vsl_forward_shared and vsl_backward_shared after any other forward are errors, and vsl_loss finds its scratch in the last
 * forward's plan.  The addressing limits (2^31 workspace floats, 2 GiB per (rows, 128) activation) apply to N T 128 and to B T 128 separately.
 * Detect the feature by the presence of the symbols: VSL_ABI_VERSION does not change for an added entry point. */
typedef struct {                       /* zero-initialise; new fields are appended */
    int32_t N;                         /* videos (>= 1)                                                                                    */
    const int32_t* video_index;        /* (B), device: video of query b.  0 <= value < N is the CALLER'S precondition: the library does not */
                                       /* read it on the host, and an index outside the range reads outside the encoding                   */
    const float* video_v_mask;         /* (N, T): per VIDEO                                                                                */
} vsl_shared_io;
/* floats of vsl_io.workspace for a shared step: the training plan with the video half sized by N, plus dCv (N, T, 128) and N + 1 + B ints of grouping */
int vsl_shared_workspace_floats(vsl_handle h, int B, int N, int T, int Lq, int Lc, int64_t* out);
int vsl_forward_shared(vsl_handle h, const vsl_io* io, const vsl_shared_io* sh, void* hip_stream);
int vsl_backward_shared(vsl_handle h, const vsl_io* io, const vsl_shared_io* sh, void* hip_stream);
/* vsl_workspace_offset for the plan of a shared step: tensors of the video half ("video_affine", "venc", "venc_*", "relu_venc_*", "d_video_affine")
 * have N T rows; added names: "d_venc_video" (dCv, (N, T, 128)), "group_start" (N + 1 int32), "group_members" (B int32) */
int64_t vsl_shared_workspace_offset(vsl_handle h, int B, int N, int T, int Lq, int Lc, const char* name);

/* compute_loss + compute_highlight_loss (VSLNet_t7.py:67-72) and their gradient seeds */
int vsl_loss(vsl_handle h, const vsl_io* io, const vsl_loss_io* l, void* hip_stream);
/* THE VIDEO RANKING LOSS: vsl_loss over GROUPS of pair rows, plus a softmax ranking term over every group's video relevances (no reference
 * counterpart).  It trains the score the coarse half of a corpus search ranks videos by -- vsl_highlight_pairs' max / mean of h_score over the valid
 * clips -- to put a query's own video in front of other videos.
 * A batch of B pair rows is cut into G contiguous groups: group g is rows group_start[g] .. group_start[g + 1] - 1 (group_start[0] = 0,
 * group_start[G] = B, every group at least one row); positive[g] is the row of the group's true (query, video) pair, every other row of the group is
 * the same query against another video.  The consistency of the two tables is the CALLER'S precondition, as with vsl_shared_io.video_index; every
 * loop is bounded by B, G and T whatever they hold.  The terms:
 *   - span: vsl_loss' CE(start) + CE(end) summed over the POSITIVE rows only, times inv_pos.  A non-positive row contributes nothing: its
 *     d_start_logits / d_end_logits rows are exactly 0 and neither its logits nor its labels are read;
 *   - highlight: vsl_loss' loss over all B rows (a sampler passes all-zero h_labels on a negative row: nothing in another video is the query's moment);
 *   - relevance r_b: the reduction of vsl_highlight_pairs over row b's valid clips (relevance = 0 max, 1 mean: the same additions in the same order;
 *     -INFINITY without a valid clip), z_b = r_b * inv_temperature;
 *   - rank: per group over its rows with a finite z: lse_g = m_g + logf(sum_b expf(z_b - m_g)) added in ascending b (m_g their maximum),
 *     l_g = lse_g - z_positive; rank = inv_groups * sum_g l_g added in ascending g.  A group whose positive row has no valid clip is SKIPPED: no term,
 *     no rank gradient, no hit;
 *   - rank gradient: d r_b = w_rank * inv_groups * inv_temperature * (expf(z_b - lse_g) - [b == positive[g]]).  max: added to d_h_score[b][t*] only,
 *     t* the first valid clip that attains the maximum; mean: d r_b / count_b added at every valid clip.  A masked clip gets the highlight seed alone
 *     (0 under the mask);
 *   - hits: the non-skipped groups whose positive row is first in the order (z descending, then the smaller row).
 * losses[5] = loc, highlight, rank, w_loc loc + w_highlight highlight + w_rank rank, the mask sum used.
 * The loss has ONE definition: the kernels are built from the device functions vsl_loss' kernels are built from.  With every group of size one and
 * inv_pos = vsl_loss_io.inv_batch, at every w_rank (l_g = 0 and d r = 0 there): losses[0], losses[1] and losses[4] are bit for bit vsl_loss'
 * losses[0], [1] and [3], and the three seeds compare equal to vsl_loss' as floats.
 * No float atomic anywhere: per-row partials go through `scratch` and are re-reduced in index order; two runs give the same bits.
 * A free-standing call like vsl_merge_topk: it touches no plan and no handle state and reads only what it is passed, so it is legal behind any
 * training or saved forward; the caller hands the seeds to vsl_backward / vsl_backward_shared / vsl_backward_accumulate through vsl_io.d_* (fused_step
 * works; vsl_io.fused_loss is simply not used on such a step).  TWO launches on the caller's stream: "group_loss_a" (one workgroup per row: the
 * log-sum-exps, the highlight partial, the relevance, its argmax and count) and "group_loss_c" (a (ceil(T / 256), B) grid writes the seeds; block (0, 0)
 * the loss values and the hits).
 * Refused by name: NULL required pointers; B, G or T below 1; G above B; T above 4096; B above 65535 (a grid dimension); seeds not all-or-none;
 * inv_temperature <= 0; relevance other than 0 or 1; a NULL label array with a non-zero weight for it (start_labels and end_labels: both or neither).
 * Labels of a positive row outside [0, T) read outside the logits, as in vsl_loss.  Detect the feature by the presence of the symbols:
 * VSL_ABI_VERSION does not change for an added entry point. */
typedef struct vsl_group_loss_io {         /* zero-initialise; new fields are appended */
    int32_t B, T, G;
    const float* h_score; const float* start_logits; const float* end_logits; const float* v_mask;   /* (B, T)                                  */
    const int64_t* start_labels; const int64_t* end_labels;   /* (B); read at positive rows only; NULL iff w_loc == 0                           */
    const int64_t* h_labels;               /* (B, T); NULL iff w_highlight == 0                                                                */
    const int32_t* group_start; const int32_t* positive;      /* (G + 1), (G), device                                                          */
    float w_loc, w_highlight, w_rank;
    float inv_pos;                         /* normaliser of the span CE: 1 / number of positive rows of the GLOBAL step                        */
    float inv_groups;                      /* normaliser of the rank term                                                                      */
    float mask_sum;                        /* as vsl_loss_io.mask_sum (<= 0: this call's own sum over all B rows)                              */
    float inv_temperature;
    int32_t relevance;                     /* 0 = max, 1 = mean: vsl_highlight_io.relevance                                                    */
    float* losses;                         /* out, 5 floats: loc, highlight, rank, total, mask_sum used                                        */
    int32_t* hits;                         /* out, nullable: number of groups whose positive row ranks first                                   */
    float* pair_relevance;                 /* out (B), nullable                                                                                */
    float* d_h_score; float* d_start_logits; float* d_end_logits;   /* out (B, T), all or none; overwritten                                    */
    float* scratch;                        /* vsl_group_loss_scratch_floats(B, G) floats, caller-owned                                         */
} vsl_group_loss_io;
/* floats of vsl_group_loss_io.scratch: ten per-row arrays (log-sum-exps, CE term, highlight numerator, mask sum, relevance, argmax, count, group, z) */
int vsl_group_loss_scratch_floats(int B, int G, int64_t* out);
int vsl_group_loss(vsl_handle h, const vsl_group_loss_io* l, void* hip_stream);
/* autograd backward of everything in vsl_forward (main_t7.py:110); needs the same io (workspace, seed) */
int vsl_backward(vsl_handle h, const vsl_io* io, void* hip_stream);
/* GRADIENT ACCUMULATION: one optimizer step over K micro-batches (no reference counterpart: main_t7.py steps once per batch).  vsl_backward_accumulate is
 * vsl_backward (sh = NULL, after vsl_forward) or vsl_backward_shared (sh = the step's vsl_shared_io, after vsl_forward_shared) with ONE difference:
 * what the call would store in io->grads is ADDED to what the bucket holds.  A step is then: the first micro-batch through vsl_backward (it overwrites:
 * nothing has to be zeroed), every further one through this call, each after its own forward.  With the GLOBAL normalisers in vsl_loss_io, the
 * micro-batch's first row as vsl_io.sample_offset and one seed for the step, a micro-batch is a data-parallel shard run in sequence: the accumulated
 * bucket is the gradient of the whole batch up to fp32 summation order.
 *   - io->grads must hold the running sum on the caller's stream (the earlier calls of the step, enqueued there);
 *   - add order: every element's new value is  previous + s,  s = what vsl_backward would have stored (the same slab sums in the same order), as one
 *     fp32 add.  After calls 0 .. K-1 the bucket holds ((g0 + g1) + g2) + ...; there is no float atomic, two runs of a step give identical bits.  With
 *     word_table = 1 the rows of the table that no word of the micro-batch touches keep their value;
 *   - fused_loss works as in vsl_backward;
 *   - fused_step applies clip + AdamW to the ACCUMULATED bucket, with the norm of the accumulated bucket (the reduction records the squares of the
 *     values it stores).  Setting it is how the caller marks the last micro-batch of the step;
 *   - early_grads_event (sh = NULL only) is allowed: the early block holds its accumulated value when the event fires;
 *   - afterwards vsl_adamw_step(norm_from_backward = 1) on that bucket is valid and takes the accumulated norm.
 * Refused: NULL grads; sh that does not match the handle's last forward (the messages of vsl_backward / vsl_backward_shared); a last forward that saved
 * nothing.  Workspace needs and plans are those of the micro-batch's own shape: a global batch whose training plan exceeds the 2^31-float limit runs as
 * micro-batches that fit.  Detect the feature by the presence of the symbol: VSL_ABI_VERSION does not change for an added entry point. */
int vsl_backward_accumulate(vsl_handle h, const vsl_io* io, const vsl_shared_io* sh /* NULL after vsl_forward */, void* hip_stream);
/* GRADIENT WITH RESPECT TO THE VIDEO FEATURES (what autograd returns as video_features.grad when the features require grad: a trainable adapter in
 * front of the model, an adversarial perturbation, a saliency map).  vsl_backward stops one product short of it: it leaves d_video_affine, the
 * gradient of VisualProjection's output, in the workspace.  This call computes
 *     d_video_features[r][c] = m(r, c) * sum_{j < 128} d_video_affine[r][j] * W[j][c],      W = video_affine.linear.conv1d.weight as (128, video_feature_dim),
 * m = the multiplier VisualProjection's dropout applied to feature (r, c) in the forward of this io (same seed, same sample_offset; 1 with
 * training = 0 or drop_rate 0): dropped features get exactly 0, padded clips get the (generally non-zero) gradient autograd gives them.
 *   - output: (B, T, video_feature_dim) fp32; after a shared step (N, T, video_feature_dim): the gradient of each VIDEO, summed over its queries in
 *     ascending b.  With video_features_bf16 it is the fp32 gradient with respect to the widened features (the call never reads the features);
 *   - legal after vsl_backward, vsl_backward_shared or vsl_backward_accumulate of the same io on the same stream, until the next forward of the
 *     handle; with accumulation each micro-batch's call gives that micro-batch's rows.  It reads io->params, io->workspace, training, seed and
 *     sample_offset, writes nothing but the output, and may be repeated (identical bits);
 *   - ONE launch on the caller's stream (ledger label "vproj_dx"), fp32-grade: the fp32-input MFMA, a 128-term fmaf chain per element.  No plan
 *     grows for it and vsl_forward / vsl_backward launch nothing for it: a caller who never asks pays nothing.
 * Refused (vsl_last_error names the reason): a NULL output; no backward since the handle's last forward; a last forward that saved nothing
 * (inference, vsl_encode_video, vsl_localize); an `sh` that does not match the last forward (the messages of vsl_backward / vsl_backward_shared); a last
 * backward that applied fused_step -- the weight this product needs has been overwritten: run the backward without it, this call, then vsl_adamw_step.
 * Detect the feature by the presence of the symbol: VSL_ABI_VERSION does not change for an added entry point. */
int vsl_input_grads(vsl_handle h, const vsl_io* io, const vsl_shared_io* sh /* NULL after vsl_forward */, float* d_video_features, void* hip_stream);
/* first float offset of the parameter block whose gradients are final when vsl_io.early_grads_event fires (== vsl_param_floats()
 * when the configuration has no such block: the rnn predictor) */
int64_t vsl_early_grad_offset(vsl_handle h);

/* test hook (tests/test_rnn_fused.py): sets the process-wide counter the fused rnn head derives its granule tags from -- 21 bits of it are the
 * tag, the bits above the generation for which a plan's granule buffers were last cleared -- so that a test can step across the wrap without two
 * million launches.  Returns the previous value.  No reference counterpart. */
uint64_t vsl_debug_rnn_launches(uint64_t n);
/* ConditionedPredictor.extract_index (layers_t7.py:355-363) */
int vsl_extract_index(vsl_handle h, const float* start_logits, const float* end_logits, int B, int T,
                      int64_t* start_index, int64_t* end_index, void* hip_stream);

/* THE K BEST MOMENTS PER QUERY: greedy selection with temporal non-maximum suppression (no reference counterpart: extract_index returns one span).
 * For sample b, L = valid_len[b] clamped into [1, T] (T without valid_len):
 *   - candidates: every span (s, e), 0 <= s <= e < L, and e - s + 1 <= max_span when max_span > 0;
 *   - score = start_logits[b][s] + end_logits[b][e], ONE fp32 addition.  extract_index ranks by softmax(sl)[s] softmax(el)[e] = exp(score - lse_s - lse_e)
 *     and the normalisers are constant per sample: the order by score is the order by that product, exact and free of exp;
 *   - order: score descending, then start ascending, then end ascending (the first maximum in row-major order, extract_index's tie rule);
 *   - K rounds; each takes the first candidate in that order that is neither chosen nor suppressed by an earlier choice;
 *   - (s, e) is suppressed by a chosen (s', e') iff, as clip intervals [s, e + 1),  inter = max(0, min(e, e') - max(s, s') + 1),
 *     uni = (e - s + 1) + (e' - s' + 1) - inter,  inter > 0 && (float)inter > nms_iou * (float)uni  (one fp32 multiply).  nms_iou = 1 suppresses
 *     nothing (plain top-K), nms_iou = 0 keeps mutually disjoint spans only;
 *   - outputs (B, K): start_index, end_index, score (the logit sum), prob = expf(score - lse_s - lse_e) with both log-sum-exps over the sample's T
 *     logits as the reference's softmax runs (nullable), and count (B) = rounds that found a candidate (nullable).  Slots from count[b] on hold
 *     -1, -1, -inf, 0.
 * Limits: 1 <= K <= 32, 1 <= T <= 4096, B >= 1, max_span >= 0, 0 <= nms_iou <= 1.  NaN logits give an unspecified choice (every loop is bounded).
 * A free-standing call like vsl_extract_index: it reads no plan and no workspace and is legal after any kind of forward; one workgroup per sample,
 * the (T, T) scores are never materialised.  Detect the feature by the presence of the symbol: VSL_ABI_VERSION does not change for an added entry point. */
typedef struct vsl_topk_io {               /* zero-initialise; new fields are appended */
    const float* start_logits; const float* end_logits;   /* (B, T) */
    const int32_t* valid_len;                             /* (B,) or NULL = T */
    int B, T, K; float nms_iou; int max_span;             /* max_span 0 = unlimited */
    int64_t* start_index; int64_t* end_index;             /* (B, K) */
    float* score; float* prob; int32_t* count;            /* (B, K), (B, K) or NULL, (B,) or NULL */
} vsl_topk_io;
int vsl_extract_topk(vsl_handle h, const vsl_topk_io* io, void* hip_stream);

/* THE K_out BEST MOMENTS OF EVERY GROUP OF TOP-K LISTS: the device-side merge behind a search over several videos (no reference counterpart).  A list is
 * what vsl_extract_topk leaves for one (query, video) pair -- K slots of (start, end, score) with a ranking `key` (normally its `prob`), `count` of them
 * filled -- and a group is every list of one query.  Per group g the call writes K_out slots:
 *   - candidates: slot k < min(count[b], K) of every list b with group_index[b] == g.  A group_index outside [0, G) puts the list in no group;
 *   - every candidate carries a tag: tag[b] (the list's video, say), b itself when `tag` is NULL, or tag[b][k] with tag_per_slot != 0 (a (B, K) array:
 *     the out_tag of an earlier merge, see below);
 *   - order: key descending, then tag ascending, then list b ascending, then slot ascending.  That is a strict total order, so the K_out first
 *     candidates are a pure function of the inputs: the same bits on every run, no atomic anywhere.  The lists need not be sorted;
 *   - outputs (G, K_out): out_tag, out_list (the b a slot came from), out_start, out_end, out_score, out_key copied from the chosen candidate, and
 *     out_count (G) = candidates written.  Slots from out_count[g] on hold -1, -1, -1, -1, -inf, 0.
 * TWO LEVELS: a corpus too large for one call is merged in chunks and the chunks' results are merged again -- the first level's outputs are the second
 * level's lists (K = the first level's K_out, count = its out_count, tag = its out_tag with tag_per_slot = 1, group_index = the group a row belongs
 * to).  When every tag occurs in exactly one first-level call and every chunk's K_out is at least the final K_out, out_tag / out_start /
 * out_end / out_score / out_key / out_count of the second level are exactly those of ONE call over all the lists: candidates that tie in key and tag sit
 * in one chunk, whose output keeps their order (out_list then numbers the second level's rows).
 * Limits: 1 <= K <= 32, 1 <= K_out <= 32, B >= 1, G >= 1; every pointer but `tag` is required.  NaN keys give an unspecified choice (every loop is
 * bounded by B, K and K_out).  A free-standing call like vsl_extract_topk: it reads no plan and no workspace and is legal after any kind of forward; one
 * workgroup per group, ONE launch on the caller's stream.  Detect the feature by the presence of the symbol: VSL_ABI_VERSION does not change for an
 * added entry point. */
typedef struct vsl_merge_io {              /* zero-initialise; new fields are appended */
    int B, K, G, K_out;
    const int64_t* start; const int64_t* end;             /* (B, K) */
    const float* score; const float* key;                 /* (B, K) */
    const int32_t* count;                                 /* (B,) */
    const int32_t* group_index;                           /* (B,), device */
    const int32_t* tag;                                   /* (B,), (B, K) with tag_per_slot, or NULL = b */
    int32_t tag_per_slot;
    int32_t* out_tag; int32_t* out_list;                  /* (G, K_out) */
    int64_t* out_start; int64_t* out_end;                 /* (G, K_out) */
    float* out_score; float* out_key;                     /* (G, K_out) */
    int32_t* out_count;                                   /* (G,) */
} vsl_merge_io;
int vsl_merge_topk(vsl_handle h, const vsl_merge_io* io, void* hip_stream);

/* SLIDING WINDOWS OVER A VIDEO OF ANY LENGTH (no reference counterpart: it resamples every video down to max_pos_len clips).  A trained model runs over
 * overlapping windows of T clips; two calls make that a device-side path.
 *
 * vsl_encode_windows: VisualProjection ONCE over the `rows` feature rows of the call, then encoder application 0 over N windows of T clips.  Window n
 * is feature rows window_row[n] .. window_row[n] + window_len[n] - 1.  The result is what vsl_encode_video writes for the materialised batch
 *     X[n][t] = features[window_row[n] + t]  for t < window_len[n],  a zero feature row otherwise,       v_mask[n][t] = t < window_len[n]
 * and the library never builds X: a clip that lies in several windows is projected once, and one launch (ledger label "window_gather") copies each
 * window's projected rows -- and, into the pad rows, the projection of a zero row, which is the bias -- into the slot the encoder reads.  The
 * encoding is bit for bit vsl_encode_video's on X at the same N and T.
 *   - window_row, window_len: (N) int32 on the DEVICE.  A source row outside [0, rows), or t >= window_len[n], is a pad row: a bad table cannot read
 *     outside the features.  window_len[n] in 1..T is the caller's precondition (0 gives an all-pad window, whose softmax over no key is the caller's
 *     problem as with an all-zero v_mask in vsl_encode_video);
 *   - outputs: video_encoding (N, T, 128) and v_mask (N, T), both written; together they are a resident encoding for vsl_localize / vsl_localize_pairs;
 *   - workspace: vsl_encode_windows_workspace_floats = the plan of vsl_encode_video at (N, T) plus rows * 128 floats;
 *   - the call marks its workspace like an inference forward (nothing saved; vsl_backward there and vsl_workspace_offset are refused).
 * Refused by name: N < 1; T outside 1 .. min(4096, max_pos_len); rows < 1; rows * video_feature_dim, rows * 128 or N * T * 128 at or above 2^31; a NULL
 * pointer.  Detect the feature by the presence of the symbols: VSL_ABI_VERSION does not change for an added entry point. */
typedef struct vsl_encode_windows_io {     /* zero-initialise; new fields are appended */
    int32_t rows, N, T;                    /* feature rows of the call ; windows ; clips per window                                            */
    const float* params;
    const float* video_features;           /* (rows, video_feature_dim) fp32, or NULL with video_features_bf16                                 */
    const uint16_t* video_features_bf16;   /* bf16 throughput mode, as vsl_io.video_features_bf16                                              */
    const int32_t* window_row;             /* (N), device: first feature row of window n                                                       */
    const int32_t* window_len;             /* (N), device: valid clips of window n                                                             */
    float* video_encoding;                 /* (N, T, 128) out                                                                                  */
    float* v_mask;                         /* (N, T) out                                                                                       */
    float* workspace;                      /* vsl_encode_windows_workspace_floats() floats                                                     */
} vsl_encode_windows_io;
int vsl_encode_windows_workspace_floats(vsl_handle h, int N, int T, int rows, int64_t* out);
int vsl_encode_windows(vsl_handle h, const vsl_encode_windows_io* io, void* hip_stream);

/* vsl_merge_windows: the K_out best moments of every GROUP of window lists in the video's own clip coordinates, with temporal NMS across the lists.  A
 * list is what vsl_extract_topk leaves for one (window, query) pair at window-local indices; a group is every window of one (query, video) pair;
 * offset[b] is the clip index of list b's window start (NULL: 0 everywhere).  Per group g:
 *   - candidates: slot k < min(count[b], K) of every list b with group_index[b] == g (a group_index outside [0, G): no group); the global span of a
 *     candidate is (start + offset[b], end + offset[b]), which must fit an int32;
 *   - order: key descending, then global start, global end, list and slot ascending -- a strict total order;
 *   - K_out rounds; each takes the first candidate in that order that is not suppressed by an earlier choice of the group;
 *   - a candidate is suppressed by a chosen span iff the two global spans are IDENTICAL (at every nms_iou: a moment two windows report is written
 *     once) or vsl_extract_topk's rule holds on the global spans (the same integers, one fp32 multiply).  nms_iou = 1 removes duplicates only;
 *   - outputs (G, K_out): out_list (the b a slot came from), out_start, out_end (global), out_score, out_key, and out_count (G) = rounds that found a
 *     candidate.  Slots from out_count[g] on hold -1, -1, -1, -inf, 0.
 * Limits, each refused by name: 1 <= K <= 32, 1 <= K_out <= 32, B >= 1, G >= 1, 0 <= nms_iou <= 1; every pointer but `offset` is required.  NaN keys
 * give an unspecified choice (every loop is bounded by B, K and K_out).  A free-standing call like vsl_merge_topk: no plan, no workspace, no atomic --
 * the same bits on every run; one workgroup per group, ONE launch on the caller's stream.  Detect the feature by the presence of the symbol. */
typedef struct vsl_merge_windows_io {      /* zero-initialise; new fields are appended */
    int B, K, G, K_out; float nms_iou;
    const int64_t* start; const int64_t* end;             /* (B, K), window-local */
    const float* score; const float* key;                 /* (B, K) */
    const int32_t* count;                                 /* (B,) */
    const int32_t* group_index;                           /* (B,), device */
    const int32_t* offset;                                /* (B,), device, or NULL = 0 */
    int32_t* out_list;                                    /* (G, K_out) */
    int64_t* out_start; int64_t* out_end;                 /* (G, K_out), global */
    float* out_score; float* out_key;                     /* (G, K_out) */
    int32_t* out_count;                                   /* (G,) */
} vsl_merge_windows_io;
int vsl_merge_windows(vsl_handle h, const vsl_merge_windows_io* io, void* hip_stream);

/* Optimizer step on the flat buckets: clip_grad_norm_(grads, clip_norm) (main_t7.py:111) followed by AdamW with decoupled
 * weight decay (build_optimizer_and_scheduler, VSLNet_t7.py:8-17: no decay for names containing "bias", "layer_norm" or
 * "LayerNorm" -- the library derives that mask from its own parameter names).  Two kernels (one with norm_from_backward), no host synchronisation: the
 * global norm stays on the device.  Semantics are torch.optim.AdamW's (the reference's transformers.AdamW no longer
 * exists; SURVEY 8c "optimizer parity unpinned"):
 *     g   = grads * min(1, clip_norm / (||grads||_2 + 1e-6))            (clip_norm <= 0: no clipping)
 *     p  *= 1 - lr * weight_decay[param]
 *     m   = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g^2
 *     p  -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * `step` is t (1-based).  exp_avg / exp_avg_sq are caller-owned buckets of vsl_param_floats() floats, zero at t = 1.
 * grad_norm_out (nullable): device float that receives the un-clipped global norm.  `grads` is not modified. */
typedef struct {
    float lr, beta1, beta2, eps, weight_decay, clip_norm;
    int32_t step;
    /* 0: torch.optim.AdamW ordering (above).  1: the historical transformers.AdamW the reference was written against
     * (VSLNet_t7.py:5,14; class removed from transformers 5.x, semantics from its published source):
     *     p -= lr * sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps) ;  then  p -= lr * weight_decay[param] * p          */
    int32_t hf_order;
    /* 1: the caller vouches that `grads` is exactly what the last vsl_backward of this handle left (no all-reduce, no scaling in
     * between: single-GPU training).  The global norm is then taken from the sums of squares the backward's final reduction
     * recorded per block instead of another pass over the bucket (one kernel less on the step's tail); the un-clipped norm agrees
     * with the two-kernel form to fp32 rounding (another summation order).  An error if `grads` is another buffer. */
    int32_t norm_from_backward;
} vsl_adamw;
int vsl_adamw_step(vsl_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   const vsl_adamw* hp, float* grad_norm_out, void* hip_stream);
/* vsl_io.fused_step: vsl_backward followed by vsl_adamw_step(params, io->grads, exp_avg, exp_avg_sq, &hp, grad_norm_out) with
 * hp.norm_from_backward = 1, as ONE call (main_t7.py:110-113 without the host in between).  `params` is normally vsl_io.params itself: every
 * kernel that reads the weights is ordered in front of the update.  io->grads still receives the (unclipped) gradients.  The library issues
 * the final reduction and the update as two launches on the caller's stream. */
typedef struct vsl_fused_step {
    float* params;
    float* exp_avg;
    float* exp_avg_sq;
    vsl_adamw hp;
    float* grad_norm_out;      /* optional */
} vsl_fused_step;

/* workspace introspection for the parity tests: float offset of a named saved activation, -1 if unknown, -2 (and vsl_last_error()) when the
 * handle's last forward was an inference forward (or vsl_encode_video / vsl_localize / vsl_encode_query / vsl_localize_pairs), which saves nothing.
 * names: "video_affine", "embedding_net", "venc", "qenc", "cq_attention", "cq_concat", "gated", "pred_s", "pred_e" */
int64_t vsl_workspace_offset(vsl_handle h, int B, int T, int Lq, int Lc, const char* name);

/* per-kernel timing with HIP events recorded on the launch stream (no reference counterpart; feeds bench.py's roofline
 * object).  select: kernel launcher name ("wgrad", "vproj_fwd", ... or "*" for all, NULL/"" = off) and resets the
 * records; read: index-th aggregated record, returns 2 past the end. */
int vsl_profile_select(vsl_handle h, const char* kernel);
int vsl_profile_read(vsl_handle h, int index, char* name, int name_cap, double* total_ms, int32_t* count);
/* the same records one launch at a time, in enqueue order (tools/critical_path.py: the step's critical-path ledger): stream = index of
 * the launch's stream in order of first appearance, start / stop = the kernel's own dispatch-packet timestamps in us relative to the first
 * record's start, host = when the host enqueued it (us since vsl_profile_select), deps = indices of the launches it was ordered behind
 * (same-stream predecessor + every cross-stream ordering point in front of it).  Returns 2 past the end. */
int vsl_profile_launch(vsl_handle h, int index, char* name, int name_cap, int32_t* stream, double* start_us, double* stop_us,
                       double* host_us, int32_t* deps /* [6] */, int32_t* ndeps);

#ifdef __cplusplus
}
#endif
#endif
