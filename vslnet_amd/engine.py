"""ctypes binding of libvslnet_hip.so (include/vslnet_hip.h) + a thin engine object.

PyTorch-ROCm tensors are used for STORAGE ONLY: every pointer handed to the library is `tensor.data_ptr()` of a
caller-owned CUDA(HIP) tensor, and all kernels are enqueued on torch's current stream.  There is no CPU fallback:
if the shared library is missing or no MI355X is visible, construction raises.
"""
import ctypes as C
import os

import torch

from .abi import (ABI_SYMBOLS, ABI_VERSION, FEATURES, PROTOTYPES, RELEVANCE, TOPM_MAX_M, CorpusMoments, LongMoments, TopkSpans, VideoRanks, VslError,  # noqa: F401
                  WindowMoments, load_library, vsl_adamw, vsl_config, vsl_encode_io, vsl_encode_query_io, vsl_encode_windows_io, vsl_fused_step,
                  vsl_group_loss_io, vsl_highlight_io, vsl_io, vsl_localize_io, vsl_loss_io, vsl_merge_io, vsl_merge_windows_io, vsl_pairs_io,
                  vsl_select_io, vsl_shared_io, vsl_topk_io)


class VideoEncoding:
    """What Engine.encode_video returns and Engine.localize reads: the shared feature encoder's output for N videos padded to T clips, and their
    clip masks.  It belongs to its T and to the parameter values it was computed with (include/vslnet_hip.h).  `owner` / `epoch` are set by
    VSLNet.encode_video: the module refuses a handle of another module or of parameters that may have changed since."""
    __slots__ = ('encoding', 'v_mask', 'N', 'T', 'owner', 'epoch')

    def __init__(self, encoding, v_mask, owner=None, epoch=None):
        self.encoding, self.v_mask = encoding, v_mask
        self.N, self.T = int(encoding.shape[0]), int(encoding.shape[1])
        self.owner, self.epoch = owner, epoch


class QueryEncoding:
    """What Engine.encode_query returns: the shared feature encoder's output for Q queries padded to Lq words (embedded at Lc chars per word), and
    their word masks.  It belongs to its Lq and Lc and to the parameter values it was computed with (include/vslnet_hip.h).  `owner` / `epoch` are
    set by VSLNet.encode_query, like VideoEncoding's."""
    __slots__ = ('encoding', 'q_mask', 'Q', 'Lq', 'Lc', 'owner', 'epoch')

    def __init__(self, encoding, q_mask, Lc, owner=None, epoch=None):
        self.encoding, self.q_mask = encoding, q_mask
        self.Q, self.Lq, self.Lc = int(encoding.shape[0]), int(encoding.shape[1]), int(Lc)
        self.owner, self.epoch = owner, epoch


class WindowEncoding(VideoEncoding):
    """What VSLNet.encode_windows returns: a VideoEncoding over ALL sliding windows of a list of videos (row n = window n; `localize` and
    `localize_pairs` take it as it is, owner / epoch / staleness as for any VideoEncoding), and where the windows lie: `video_of_window`,
    `offset_of_window` (the window's first clip in its video) and `window_len` as (N,) int32 device tensors, `lengths` (clips per video) and
    `first_window` (V + 1 prefix sums: video v owns windows first_window[v] .. first_window[v + 1] - 1) as numpy arrays, `window` and `stride`."""
    __slots__ = ('video_of_window', 'offset_of_window', 'window_len', 'lengths', 'first_window', 'window', 'stride')

    def __init__(self, encoding, v_mask, video_of_window, offset_of_window, window_len, lengths, first_window, window, stride, owner=None, epoch=None):
        super().__init__(encoding, v_mask, owner=owner, epoch=epoch)
        self.video_of_window, self.offset_of_window, self.window_len = video_of_window, offset_of_window, window_len
        self.lengths, self.first_window, self.window, self.stride = lengths, first_window, int(window), int(stride)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, dtype, shape, name):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_cuda or not t.is_contiguous():
        raise ValueError('%s: expected contiguous cuda %s %s, got %s %s on %s' %
                         (name, dtype, tuple(shape), t.dtype, tuple(t.shape), t.device))


_HW_QUEUE_WARNED = False


def check_hw_queues():
    """A process group over RCCL brings its own streams; with fewer than 8 hardware queues the library's two side streams then share a
    queue with another stream and the fork / join overlap of the step is silently lost (measured: 1.25 -> 1.51 ms per step).  The
    variable only counts if it was in the environment before the process initialised HIP -- the library cannot enforce that, so it refuses
    to run in the state it can detect AND that costs: an nccl (= RCCL) group of more than one rank with GPU_MAX_HW_QUEUES below 8 or set too
    late.  Anything else -- a gloo group, one rank, an embedding application that initialised HIP first -- is a performance note, printed once;
    VSL_ALLOW_FEW_HW_QUEUES=1 turns the refusal into that note as well."""
    global _HW_QUEUE_WARNED
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    import vslnet_amd
    try:
        q = int(os.environ.get('GPU_MAX_HW_QUEUES', '0'))
    except ValueError:
        q = 0
    if q >= 8 and not vslnet_amd.QUEUES_SET_LATE:
        return
    msg = ('GPU_MAX_HW_QUEUES=%s%s while a torch.distributed process group exists: the step needs 8 hardware queues beside '
           "RCCL's streams.  Export GPU_MAX_HW_QUEUES=8 before the process starts (or import vslnet_amd before the first CUDA call)"
           % (os.environ.get('GPU_MAX_HW_QUEUES'), ' (set after HIP was initialised)' if vslnet_amd.QUEUES_SET_LATE else ''))
    rccl_multi = dist.get_backend() == 'nccl' and dist.get_world_size() > 1
    if rccl_multi and os.environ.get('VSL_ALLOW_FEW_HW_QUEUES') != '1':
        raise VslError(msg)
    if not _HW_QUEUE_WARNED:
        _HW_QUEUE_WARNED = True
        import warnings
        warnings.warn('vslnet_amd: ' + msg + ' -- continuing (%s)' % ('VSL_ALLOW_FEW_HW_QUEUES=1' if rccl_multi else 'no multi-rank RCCL group: nothing to lose'))


def _c_int(who, **values):
    """(ctypes would wrap them: max_span = 2 ** 32 must not arrive as 0 = unlimited; the library checks the ranges)"""
    for name, v in values.items():
        if not -2 ** 31 <= v < 2 ** 31:
            raise ValueError('%s: %s=%d is not a C int' % (who, name, v))


class Engine:
    """One `vsl_handle` + caller-owned buffers.  Mirrors what VSLNet.__init__ / forward / backward need."""
    h = None                                                # (until vsl_create has succeeded: what __del__ of a half-built engine finds)

    def __init__(self, configs, device=None, word_table=None):
        """`word_table=True` (or configs.word_table): WordEmbedding(word_vectors=None), the trainable nn.Embedding branch
        (layers_t7.py:36); forward() then takes pad_vec = glove_vec = None."""
        if not torch.cuda.is_available():
            raise VslError('vslnet_amd needs an MI355X (gfx950) visible to PyTorch-ROCm; there is no CPU fallback')
        check_hw_queues()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.lib = load_library()
        # vsl_io.fused_loss / fused_step (ABI 8): an older build loaded through VSLNET_HIP_LIB for an A/B run takes the separate calls instead
        self.has_fused_io = hasattr(self.lib, 'vsl_abi_version') and self.lib.vsl_abi_version() >= 8
        # has_inference, has_shared_video, ...: what an older build lacks, the methods that need it refuse (_need).  Plain attributes: tests clear them
        for flag, (symbols, _) in FEATURES.items():
            setattr(self, 'has_' + flag, all(hasattr(self.lib, s) for s in symbols))
        self.use_inference = True                           # `False` keeps the module's no_grad path on the saved path on a current build too (A/B runs, tests)
        self._group_scratch = {}                        # (B, G) -> the call's scratch
        self.inference_forwards = 0                          # inference forwards issued so far (tests, tools/infer_rate.py)
        pred = {'rnn': 0, 'transformer': 1}.get(configs.predictor)
        if pred is None:
            raise ValueError('unknown predictor %r' % (configs.predictor,))
        self.cfg = vsl_config(int(configs.dim), int(configs.num_heads), int(configs.max_pos_len),
                              int(configs.video_feature_dim), int(configs.word_dim), int(configs.char_dim),
                              int(configs.word_size), int(configs.char_size), pred, float(configs.drop_rate),
                              int(bool(getattr(configs, 'word_table', False) if word_table is None else word_table)))
        self.configs = configs
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            if self.lib.vsl_create(C.byref(self.cfg), C.byref(h)):
                msg = self.lib.vsl_last_error().decode()
                if 'not implemented' in msg:
                    raise NotImplementedError(msg)
                if 'not a multiple of attention heads' in msg:
                    raise AssertionError(msg)               # same condition the reference asserts (layers_t7.py:146)
                raise VslError(msg)
        self.h = h
        self.param_floats = int(self.lib.vsl_param_floats(h))
        self.layout = []                                    # (name, offset, numel, shape)
        name = C.create_string_buffer(256)
        off, num, nd = C.c_int64(), C.c_int64(), C.c_int32()
        dims = (C.c_int64 * 4)()
        for i in range(self.lib.vsl_param_count(h)):
            self._call(self.lib.vsl_param_info(h, i, name, 256, C.byref(off), C.byref(num), C.byref(nd), dims))
            self.layout.append((name.value.decode(), off.value, num.value, tuple(dims[j] for j in range(nd.value))))
        self._ws, self._grown = None, False                 # the one shared workspace (workspace())
        self._last = None                                   # the vsl_io of the last forward (a marker with inference = 1 behind a call that saved nothing)
        self._last_ws = None                                # the workspace it ran in (None where nothing was saved)
        self._last_shared = None                            # the vsl_shared_io of the last forward when that was forward_shared (loss / backward / ws_view dispatch on it)
        self._keep = None                                   # every tensor the last call's io points to, alive until the backward
        self._pending_loss = None                           # a lazy loss(): (vsl_loss_io, the forward's vsl_io, its tensors)

    def __del__(self):
        try:
            if self.h:
                self.lib.vsl_destroy(self.h)
        except Exception:
            pass

    def _call(self, rc):
        if rc:
            msg = self.lib.vsl_last_error().decode()
            if 'exceeds max_pos_len' in msg:
                raise IndexError(msg)                       # the reference raises IndexError from nn.Embedding here
            raise VslError(msg)

    def _need(self, flag):
        """The refusal of a method whose entry points the loaded library lacks (abi.FEATURES)."""
        if not getattr(self, 'has_' + flag):
            raise VslError(FEATURES[flag][1])

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- flat parameter bucket helpers -------------------------------------------------------------------
    def new_flat(self):
        return torch.zeros(self.param_floats, dtype=torch.float32, device=self.device)

    def views(self, flat):
        return {n: flat[o:o + k].view(shp) for n, o, k, shp in self.layout}

    # ---- the workspace: floats per shape and call, one buffer ----------------------------------------------
    def _floats(self, query, *shape):
        """What the library's `query` (one of its *_workspace_floats) answers for this shape."""
        n = C.c_int64()
        with torch.cuda.device(self.device):
            self._call(query(self.h, *shape, C.byref(n)))
        return int(n.value)

    def inference_workspace_floats(self, B, T, Lq, Lc):
        """Floats an inference forward of this shape needs (the forward-only plan; vslnet_hip.h)."""
        self._need('inference')
        return self._floats(self.lib.vsl_inference_workspace_floats, B, T, Lq, Lc)

    def workspace_floats(self, B, T, Lq, Lc):
        """Floats a training (or saved-path evaluation) forward + backward of this shape needs."""
        return self._floats(self.lib.vsl_workspace_floats, B, T, Lq, Lc)

    def encode_workspace_floats(self, N, T):
        """Floats an encode_video call of N videos padded to T clips needs (operand packs + one encoder application's scratch)."""
        self._need('shared_video')
        return self._floats(self.lib.vsl_encode_workspace_floats, N, T)

    def localize_workspace_floats(self, B, T, Lq, Lc):
        """Floats a localize call of this shape needs (the inference plan without a video pass + the (B, T) gathered mask)."""
        self._need('shared_video')
        return self._floats(self.lib.vsl_localize_workspace_floats, B, T, Lq, Lc)

    def shared_workspace_floats(self, B, N, T, Lq, Lc):
        """Floats a shared training step of B queries over N videos needs (the training plan with the video half sized by N, + dCv and the grouping)."""
        self._need('shared_train')
        return self._floats(self.lib.vsl_shared_workspace_floats, B, N, T, Lq, Lc)

    def encode_windows_workspace_floats(self, N, T, rows):
        """Floats an encode_windows call of N windows of T clips over `rows` feature rows needs (the encode plan of (N, T) + rows * 128)."""
        self._need('windows')
        return self._floats(self.lib.vsl_encode_windows_workspace_floats, int(N), int(T), int(rows))

    def encode_query_workspace_floats(self, Q, Lq, Lc):
        """Floats an encode_query call of Q queries padded to Lq words of Lc chars needs (operand packs + the query branch's scratch)."""
        self._need('query_encoding')
        return self._floats(self.lib.vsl_encode_query_workspace_floats, Q, Lq, Lc)

    def pairs_workspace_floats(self, B, T, Lq):
        """Floats a localize_pairs call of this shape needs (the localize plan without the query branch's scratch)."""
        self._need('query_encoding')
        return self._floats(self.lib.vsl_pairs_workspace_floats, B, T, Lq)

    def _grow_ws(self, n):
        """The one shared workspace (see workspace()), grown to at least `n` floats."""
        if self._ws is None or self._ws.numel() < n:
            # drop EVERY reference to the old one first (the last forward's io / keep-alive tuple hold it too): old and new must not
            # coexist at the growth peak beside an HBM-resident dataset
            self._ws = None
            self._last = self._last_ws = self._keep = self._last_shared = None
            self._ws = torch.empty(int(n * 1.25) if self._grown else n, dtype=torch.float32, device=self.device)
            self._grown = True
        return self._ws

    def workspace(self, B, T, Lq, Lc, inference=False):
        """ONE caller-owned workspace, grown to the largest shape seen: its contents only live from a forward to the
        backward of the same batch, and the collate narrows every batch to its own max T / Lq / Lc, so real-data training
        visits hundreds of shapes -- a workspace per shape would grow without bound beside the HBM-resident dataset.
        Inference forwards share it: their plan is a fraction of the training plan of the same shape, so they only ever grow it for a
        shape training has not seen."""
        return self._grow_ws(self._floats(self.lib.vsl_inference_workspace_floats if inference else self.lib.vsl_workspace_floats, B, T, Lq, Lc))

    def ws_view(self, name, shape):
        """Saved activation `name` of the LAST forward as a tensor view (parity tests)."""
        io = self._last
        if io is not None and io.inference:
            raise VslError('ws_view(%r): the last forward was an inference forward (or encode_video / localize), which saves nothing' % (name,))
        if self._last_shared is not None:                   # the plan of a shared step: the video half's tensors have N T rows
            off = self.lib.vsl_shared_workspace_offset(self.h, io.B, self._last_shared.N, io.T, io.Lq, io.Lc, name.encode())
        else:
            off = self.lib.vsl_workspace_offset(self.h, io.B, io.T, io.Lq, io.Lc, name.encode())
        if off < 0:
            raise KeyError(name)
        n = 1
        for s in shape:
            n *= s
        return self._last_ws[off:off + n].view(shape)

    # ---- the checks the calls share: each returns what its caller hands to the library -----------------------
    def _check_query(self, B, Lq, Lc, word_ids, char_ids, q_mask, pad_vec, glove_vec):
        """The query side of a call -> the (pad_vec, glove_vec) it uses."""
        _chk(word_ids, torch.int64, (B, Lq), 'word_ids')
        _chk(char_ids, torch.int64, (B, Lq, Lc), 'char_ids')
        _chk(q_mask, torch.float32, (B, Lq), 'q_mask')
        if self.cfg.word_table:
            return None, None                           # rows 0, 1, 2.. of the trainable table inside `flat` stand in
        _chk(pad_vec, torch.float32, (1, self.cfg.word_dim), 'pad_vec')
        _chk(glove_vec, torch.float32, (self.cfg.word_size - 2, self.cfg.word_dim), 'glove_vec')
        return pad_vec, glove_vec

    def _check_features(self, feats, rows):
        """The video features of a call, `rows` + (video_feature_dim,) in fp32 or bf16 -> the (video_features, video_features_bf16) pointer pair."""
        bf16 = feats.dtype == torch.bfloat16
        _chk(feats, torch.bfloat16 if bf16 else torch.float32, tuple(rows) + (self.cfg.video_feature_dim,), 'video_features')
        return (None, _ptr(feats)) if bf16 else (_ptr(feats), None)

    def _index(self, who, index, n, name, holder):
        """An index into a batch or an encoding of `n` entries: a device tensor is trusted (no synchronising read), anything else range-checked and
        uploaded as int32."""
        if isinstance(index, torch.Tensor) and index.is_cuda:
            return index.to(torch.int32).contiguous()
        host = torch.as_tensor(index).to(torch.int64).reshape(-1)
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= n):
            raise ValueError('%s: %s out of range: values in [%d, %d], %s' % (who, name, int(host.min()), int(host.max()), holder % n))
        return host.to(torch.int32).to(self.device)

    def _check_spans(self, who, spans, group_index, G, k_out):
        """The TopkSpans of B lists a merge reads and their groups -> (B, K, G, k_out)."""
        if spans.prob is None:
            raise ValueError('%s: the spans carry no prob to rank by (extract_topk(want_prob=True))' % who)
        B, K = spans.start.shape
        G, k_out = int(G), int(k_out)
        _c_int(who, G=G, k_out=k_out)
        _chk(spans.start, torch.int64, (B, K), 'spans.start')
        _chk(spans.end, torch.int64, (B, K), 'spans.end')
        _chk(spans.score, torch.float32, (B, K), 'spans.score')
        _chk(spans.prob, torch.float32, (B, K), 'spans.prob')
        _chk(spans.count, torch.int32, (B,), 'spans.count')
        _chk(group_index, torch.int32, (B,), 'group_index')
        return B, K, G, k_out

    def _check_scores(self, scores, start_logits, end_logits, v_mask):
        """Explicit outputs handed to loss() / group_loss() in place of the last forward's -> (B, T, their four pointers)."""
        B, T = scores.shape
        for t, nm in ((scores, 'scores'), (start_logits, 'start_logits'), (end_logits, 'end_logits'), (v_mask, 'mask')):
            _chk(t, torch.float32, (B, T), nm)
        return B, T, (_ptr(scores), _ptr(start_logits), _ptr(end_logits), _ptr(v_mask))

    def _out3(self, B, T):
        """(3, B, T): h_score / start_logits / end_logits of a forward, or their three gradient seeds."""
        return torch.empty(3, B, T, dtype=torch.float32, device=self.device)

    # ---- the three calls ------------------------------------------------------------------------------------
    def _train_io(self, flat, pad_vec, glove_vec, word_ids, char_ids, feats, v_mask, q_mask, out, ws, training, seed):
        """The vsl_io of forward() / forward_shared() over checked arguments (`feats`: _check_features' pointer pair)."""
        io = vsl_io()
        io.B, io.T = out.shape[1:]
        io.Lq, io.Lc = char_ids.shape[1:]
        io.params, io.pad_vec, io.glove_vec = _ptr(flat), _ptr(pad_vec), _ptr(glove_vec)
        io.word_ids, io.char_ids = _ptr(word_ids), _ptr(char_ids)
        io.video_features, io.video_features_bf16 = feats
        io.v_mask, io.q_mask = _ptr(v_mask), _ptr(q_mask)
        io.h_score, io.start_logits, io.end_logits = _ptr(out[0]), _ptr(out[1]), _ptr(out[2])
        io.workspace = _ptr(ws)
        io.training, io.seed = int(bool(training)), int(seed) & 0xFFFFFFFFFFFFFFFF
        return io

    def forward(self, flat, pad_vec, glove_vec, word_ids, char_ids, vfeats, v_mask, q_mask, training=False, seed=0,
                sample_offset=0, inference=False):
        """`inference=True`: a forward that will not be differentiated (vsl_io.inference): kernels that save nothing, the forward-only
        workspace plan, the same bits as `training=False`.  It overwrites the workspace, so the saves of an earlier training forward are gone:
        backward() and ws_view() raise until the next saved-path forward.  Excludes `training`.
        `sample_offset`: index of this shard's first sample in the global batch (data parallel; vslnet_hip.h).
        `vfeats` in torch.bfloat16 selects the bf16 THROUGHPUT mode (vsl_io.video_features_bf16): bf16 features in HBM and a
        bf16-MFMA VisualProjection; everything downstream stays fp32.  Not the parity path.
        (Round 6 removed vsl_io.arithmetic, the one-product mode of VisualProjection and the weight gradients: it measured +0.5 % for a 5e-2
        logit tolerance, and its measured ceiling -- every conv-block GEMM as one product too -- was 1.07 x; profiles/r05_notes.md section 9.)"""
        if inference and training:
            raise ValueError('inference=True and training=True exclude each other (the inference kernels have no dropout)')
        if inference:
            self._need('inference')
        B, T, Dv = vfeats.shape
        Lq, Lc = char_ids.shape[1], char_ids.shape[2]
        _chk(flat, torch.float32, (self.param_floats,), 'params')
        feats = self._check_features(vfeats, (B, T))
        _chk(v_mask, torch.float32, (B, T), 'v_mask')
        pad_vec, glove_vec = self._check_query(B, Lq, Lc, word_ids, char_ids, q_mask, pad_vec, glove_vec)
        self._flush_loss()                              # before anything touches the workspace: a pending lazy loss points into it (loss_scratch)
        ws = self.workspace(B, T, Lq, Lc, inference=inference)
        out = self._out3(B, T)
        io = self._train_io(flat, pad_vec, glove_vec, word_ids, char_ids, feats, v_mask, q_mask, out, ws, training, seed)
        io.sample_offset, io.inference = int(sample_offset), int(bool(inference))
        self._call(self.lib.vsl_forward(self.h, C.byref(io), self._stream()))
        self._last, self._last_ws, self._last_shared = io, ws, None      # (io.inference marks it: backward() and ws_view() raise on an inference forward)
        self.inference_forwards += int(bool(inference))
        # keep every tensor the io struct points to alive until the backward
        self._keep = (flat, pad_vec, glove_vec, word_ids, char_ids, vfeats, v_mask, q_mask, out, ws)
        return out[0], out[1], out[2]

    # ---- training through a shared video encoding: N videos, B queries per step -----------------------------
    def forward_shared(self, flat, pad_vec, glove_vec, word_ids, char_ids, video_features, video_v_mask, q_mask, video_index, training=True, seed=0):
        """forward() over N videos and B queries, query b paired with video video_index[b]: VisualProjection and the video pass of the feature
        encoder run on the (N, T, video_feature_dim) features once, everything else on B samples.  -> (h_score, start_logits, end_logits), each (B, T).
        loss() and backward() then work as after forward() (backward() runs the video half's backward on N T rows and sums the encoding's gradient
        over each video's queries in ascending b: deterministic).  The dropout of the video half draws ONE mask per video (include/vslnet_hip.h): at
        drop_rate 0 the step is the ordinary one on the replicated batch, otherwise a different but equally valid stochastic estimate.
        `video_v_mask` is the (N, T) per-video mask; the (B, T) per-query mask is built here.  `video_index` as a list / numpy array / CPU tensor
        is range-checked and uploaded as int32; a DEVICE tensor (int32 or int64) is trusted.  `training=False`: the saved evaluation path."""
        self._need('shared_train')
        if video_features.dim() != 3 or video_features.shape[0] < 1:
            raise ValueError('forward_shared: video_features must be (N, T, video_feature_dim) with N >= 1 videos, got %s' % (tuple(video_features.shape),))
        N, T, Dv = video_features.shape
        B, Lq, Lc = char_ids.shape
        vidx = self._index('forward_shared', video_index, N, 'video_index', 'the batch holds %d videos')
        _chk(vidx, torch.int32, (B,), 'video_index')
        _chk(flat, torch.float32, (self.param_floats,), 'params')
        feats = self._check_features(video_features, (N, T))
        _chk(video_v_mask, torch.float32, (N, T), 'video_v_mask')
        pad_vec, glove_vec = self._check_query(B, Lq, Lc, word_ids, char_ids, q_mask, pad_vec, glove_vec)
        self._flush_loss()
        ws = self._grow_ws(self.shared_workspace_floats(B, N, T, Lq, Lc))
        v_mask = video_v_mask.index_select(0, vidx.long()).contiguous()       # the (B, T) per-query mask
        out = self._out3(B, T)
        io = self._train_io(flat, pad_vec, glove_vec, word_ids, char_ids, feats, v_mask, q_mask, out, ws, training, seed)
        sh = vsl_shared_io()
        sh.N, sh.video_index, sh.video_v_mask = N, _ptr(vidx), _ptr(video_v_mask)
        self._call(self.lib.vsl_forward_shared(self.h, C.byref(io), C.byref(sh), self._stream()))
        self._last, self._last_ws, self._last_shared = io, ws, sh
        self._keep = (flat, pad_vec, glove_vec, word_ids, char_ids, video_features, video_v_mask, v_mask, vidx, q_mask, out, ws)
        return out[0], out[1], out[2]

    # ---- evaluation only: resident encodings and what reads them ---------------------------------------------
    def _eval_call(self, entry, io, keep):
        """Issue an evaluation-only call.  It ran in the shared workspace: whatever an earlier training forward saved there is gone, so backward()
        and ws_view() raise until the next saved-path forward (a marker in place of that forward's io, as after forward(inference=True))."""
        self._call(entry(self.h, C.byref(io), self._stream()))
        mark = vsl_io()
        mark.inference = 1
        self._last, self._last_ws, self._keep, self._last_shared = mark, None, keep, None

    def encode_video(self, flat, vfeats, v_mask):
        """VisualProjection + the video pass of the shared feature encoder for N videos, once: -> VideoEncoding (encoding (N, T, 128), v_mask (N, T)).
        No dropout, nothing saved.  `vfeats` in torch.bfloat16 selects the bf16 throughput mode, as in forward().  The encoding is the `venc`
        of forward() on these videos, bit for bit, and belongs to this T and to these parameter values."""
        self._need('shared_video')
        if vfeats.dim() != 3 or vfeats.shape[0] < 1:
            raise ValueError('encode_video: video_features must be (N, T, video_feature_dim) with N >= 1 videos, got %s' % (tuple(vfeats.shape),))
        N, T, Dv = vfeats.shape
        _chk(flat, torch.float32, (self.param_floats,), 'params')
        feats = self._check_features(vfeats, (N, T))
        _chk(v_mask, torch.float32, (N, T), 'v_mask')
        self._flush_loss()
        ws = self._grow_ws(self.encode_workspace_floats(N, T))
        enc = torch.empty(N, T, 128, dtype=torch.float32, device=self.device)
        io = vsl_encode_io()
        io.N, io.T = N, T
        io.params = _ptr(flat)
        io.video_features, io.video_features_bf16 = feats
        io.v_mask, io.video_encoding, io.workspace = _ptr(v_mask), _ptr(enc), _ptr(ws)
        self._eval_call(self.lib.vsl_encode_video, io, (flat, vfeats, v_mask, enc, ws))
        return VideoEncoding(enc, v_mask)

    def encode_windows(self, flat, feats, window_row, window_len, T, out=None, out_mask=None):
        """VisualProjection ONCE over the (rows, video_feature_dim) feature rows `feats`, then the video pass of the shared feature encoder over N
        windows of T clips: window n is rows window_row[n] .. window_row[n] + window_len[n] - 1, zero feature rows behind its length
        (include/vslnet_hip.h, vsl_encode_windows).  -> VideoEncoding (encoding (N, T, 128), v_mask (N, T) = t < window_len[n]): the bits of
        encode_video on the materialised zero-padded windows, which are never built.  `window_row` / `window_len`: (N,) int32 DEVICE tensors; a row
        outside the features is treated as padding.  `feats` in torch.bfloat16 selects the bf16 throughput mode.  `out` / `out_mask`: contiguous
        fp32 cuda tensors of those shapes to write into (slices of a larger encoding)."""
        self._need('windows')
        if feats.dim() != 2:
            raise ValueError('encode_windows: the features must be (rows, video_feature_dim), got %s' % (tuple(feats.shape),))
        rows, N, T = int(feats.shape[0]), int(window_row.numel()), int(T)
        _chk(flat, torch.float32, (self.param_floats,), 'params')
        feat_ptrs = self._check_features(feats, (rows,))
        _chk(window_row, torch.int32, (N,), 'window_row')
        _chk(window_len, torch.int32, (N,), 'window_len')
        self._flush_loss()
        ws = self._grow_ws(self.encode_windows_workspace_floats(N, T, rows))
        enc = torch.empty(N, T, 128, dtype=torch.float32, device=self.device) if out is None else out
        mask = torch.empty(N, T, dtype=torch.float32, device=self.device) if out_mask is None else out_mask
        _chk(enc, torch.float32, (N, T, 128), 'out')
        _chk(mask, torch.float32, (N, T), 'out_mask')
        io = vsl_encode_windows_io()
        io.rows, io.N, io.T = rows, N, T
        io.params = _ptr(flat)
        io.video_features, io.video_features_bf16 = feat_ptrs
        io.window_row, io.window_len = _ptr(window_row), _ptr(window_len)
        io.video_encoding, io.v_mask, io.workspace = _ptr(enc), _ptr(mask), _ptr(ws)
        self._eval_call(self.lib.vsl_encode_windows, io, (flat, feats, window_row, window_len, enc, mask, ws))
        return VideoEncoding(enc, mask)

    def merge_windows(self, spans, group_index, G, k_out, offset=None, nms_iou=0.5):
        """The k_out best moments of every group of WINDOW lists, in the video's own clips, with temporal NMS across the lists (include/vslnet_hip.h,
        vsl_merge_windows; the written specification: vslnet_amd.spans.merge_windows_reference) -> WindowMoments.  `spans`: a TopkSpans of B lists at
        window-local indices (extract_topk(want_prob=True); the ranking key is its `prob`); `group_index` (B,) int32 on the device: the (query, video)
        pair of list b, a value outside [0, G) drops the list; `offset` (B,) int32 on the device: the first clip of list b's window (None: 0).  Two
        candidates at the same global span are reported once at every nms_iou."""
        self._need('windows')
        B, K, G, k_out = self._check_spans('merge_windows', spans, group_index, G, k_out)
        if offset is not None:
            _chk(offset, torch.int32, (B,), 'offset')
        n = max(G, 0), max(k_out, 0)
        lst = torch.empty(n, dtype=torch.int32, device=self.device)
        i64 = torch.empty((2,) + n, dtype=torch.int64, device=self.device)
        f32 = torch.empty((2,) + n, dtype=torch.float32, device=self.device)
        count = torch.empty(n[0], dtype=torch.int32, device=self.device)
        io = vsl_merge_windows_io(B, K, G, k_out, float(nms_iou), spans.start.data_ptr(), spans.end.data_ptr(), spans.score.data_ptr(),
                                  spans.prob.data_ptr(), spans.count.data_ptr(), group_index.data_ptr(), offset.data_ptr() if offset is not None else None,
                                  lst.data_ptr(), i64[0].data_ptr(), i64[1].data_ptr(), f32[0].data_ptr(), f32[1].data_ptr(), count.data_ptr())
        self._call(self.lib.vsl_merge_windows(self.h, C.byref(io), self._stream()))
        return WindowMoments(lst, i64[0], i64[1], f32[0], f32[1], count)

    def encode_query(self, flat, pad_vec, glove_vec, word_ids, char_ids, q_mask):
        """The word + char embedding, the Embedding linear and the query pass of the shared feature encoder for Q queries, once: -> QueryEncoding
        (encoding (Q, Lq, 128), q_mask (Q, Lq)).  No dropout, nothing saved.  The encoding is the `qenc` of forward() on these queries, bit for bit,
        and belongs to this Lq / Lc and to these parameter values."""
        self._need('query_encoding')
        if char_ids.dim() != 3 or char_ids.shape[0] < 1:
            raise ValueError('encode_query: char_ids must be (Q, Lq, Lc) with Q >= 1 queries, got %s' % (tuple(char_ids.shape),))
        Q, Lq, Lc = char_ids.shape
        _chk(flat, torch.float32, (self.param_floats,), 'params')
        pad_vec, glove_vec = self._check_query(Q, Lq, Lc, word_ids, char_ids, q_mask, pad_vec, glove_vec)
        self._flush_loss()
        ws = self._grow_ws(self.encode_query_workspace_floats(Q, Lq, Lc))
        enc = torch.empty(Q, Lq, 128, dtype=torch.float32, device=self.device)
        io = vsl_encode_query_io()
        io.Q, io.Lq, io.Lc = Q, Lq, Lc
        io.params, io.pad_vec, io.glove_vec = _ptr(flat), _ptr(pad_vec), _ptr(glove_vec)
        io.word_ids, io.char_ids, io.q_mask = _ptr(word_ids), _ptr(char_ids), _ptr(q_mask)
        io.query_encoding, io.workspace = _ptr(enc), _ptr(ws)
        self._eval_call(self.lib.vsl_encode_query, io, (flat, pad_vec, glove_vec, word_ids, char_ids, q_mask, enc, ws))
        return QueryEncoding(enc, q_mask, Lc)

    def _pairs(self, who, p, flat, venc, qenc, video_index, query_index):
        """What localize_pairs and highlight_pairs share: the checks of the two resident encodings and of the pairs' indices (host values are
        range-checked, device tensors trusted), and the vsl_pairs_io `p` up to its outputs and its workspace.  -> (vidx, qidx), B = vidx.numel()."""
        if not isinstance(venc, VideoEncoding):
            raise TypeError('%s: venc must be the VideoEncoding that encode_video returned' % who)
        if not isinstance(qenc, QueryEncoding):
            raise TypeError('%s: qenc must be the QueryEncoding that encode_query returned' % who)
        N, T, Q, Lq = venc.N, venc.T, qenc.Q, qenc.Lq
        vidx = self._index(who, video_index, N, 'video_index', 'the encoding holds %d videos')
        qidx = self._index(who, query_index, Q, 'query_index', 'the encoding holds %d queries')
        B = int(vidx.numel())
        if B < 1:
            raise ValueError('%s: no pairs' % who)
        _chk(vidx, torch.int32, (B,), 'video_index')
        _chk(qidx, torch.int32, (B,), 'query_index')
        _chk(flat, torch.float32, (self.param_floats,), 'params')
        _chk(venc.encoding, torch.float32, (N, T, 128), 'video encoding')
        _chk(venc.v_mask, torch.float32, (N, T), 'v_mask')
        _chk(qenc.encoding, torch.float32, (Q, Lq, 128), 'query encoding')
        _chk(qenc.q_mask, torch.float32, (Q, Lq), 'q_mask')
        p.B, p.T, p.Lq, p.N, p.Q = B, T, Lq, N, Q
        p.params = _ptr(flat)
        p.video_encoding, p.v_mask, p.query_encoding, p.q_mask = _ptr(venc.encoding), _ptr(venc.v_mask), _ptr(qenc.encoding), _ptr(qenc.q_mask)
        p.video_index, p.query_index = _ptr(vidx), _ptr(qidx)
        return vidx, qidx

    def localize_pairs(self, flat, venc, qenc, video_index, query_index):
        """localize() with no query branch: pair b is query query_index[b] of the resident QueryEncoding `qenc` in video video_index[b] of the resident
        VideoEncoding `venc`.  -> (h_score, start_logits, end_logits), each (B, venc.T): what localize() returns for word_ids[query_index],
        char_ids[query_index], q_mask[query_index] -- bit for bit where the query encoding does not depend on the query's position in its batch
        (include/vslnet_hip.h).  Indices as in localize(): host values are range-checked, device tensors trusted.
        `flat` must hold the parameter values both encodings were computed with (VSLNet.localize_pairs checks that through the handles' epochs)."""
        self._need('query_encoding')
        io = vsl_pairs_io()
        vidx, qidx = self._pairs('localize_pairs', io, flat, venc, qenc, video_index, query_index)
        self._flush_loss()
        ws = self._grow_ws(self.pairs_workspace_floats(io.B, io.T, io.Lq))
        out = self._out3(io.B, io.T)
        io.h_score, io.start_logits, io.end_logits = _ptr(out[0]), _ptr(out[1]), _ptr(out[2])
        io.workspace = _ptr(ws)
        self._eval_call(self.lib.vsl_localize_pairs, io, (flat, venc, qenc, vidx, qidx, out, ws))
        return out[0], out[1], out[2]

    def highlight_pairs(self, flat, venc, qenc, video_index, query_index, relevance='max', out=None, ld=0, h_score=None):
        """localize_pairs() that stops behind the highlight layer, plus one relevance per pair (include/vslnet_hip.h, vsl_highlight_pairs; the written
        specification: vslnet_amd.spans.pair_relevance_reference): 'max' / 'mean' of the pair's h_score over its valid clips, -inf without one.
        -> `out`.  ld == 0: out is (B,) (allocated when None).  ld >= venc.N: out is a caller-owned (Q, ld) fp32 matrix and pair b goes to
        out[query_index[b], video_index[b]] -- a relevance matrix filled chunk by chunk.  `h_score`: an optional (B, T) buffer that receives the
        scores, bit for bit those of localize_pairs.  Indices as in localize_pairs: host values are range-checked, device tensors trusted."""
        self._need('video_ranking')
        self._need('query_encoding')
        if relevance not in RELEVANCE:
            raise ValueError("highlight_pairs: relevance must be 'max' or 'mean', got %r" % (relevance,))
        io = vsl_highlight_io()
        p = io.pairs
        vidx, qidx = self._pairs('highlight_pairs', p, flat, venc, qenc, video_index, query_index)
        B, T, ld = p.B, p.T, int(ld)
        if not 0 <= ld < 2 ** 31:
            raise ValueError('highlight_pairs: ld=%d is not a non-negative C int' % ld)
        if ld == 0:
            if out is None:
                out = torch.empty(B, dtype=torch.float32, device=self.device)
            _chk(out, torch.float32, (B,), 'out')
        else:
            if out is None:
                raise ValueError('highlight_pairs: ld > 0 writes into a (Q, ld) matrix: pass it as out')
            _chk(out, torch.float32, (p.Q, ld), 'out')     # (ld < N: the library refuses it by name)
        if h_score is not None:
            _chk(h_score, torch.float32, (B, T), 'h_score')
        self._flush_loss()
        ws = self._grow_ws(self.pairs_workspace_floats(B, T, p.Lq))
        p.h_score, p.workspace = _ptr(h_score), _ptr(ws)
        io.relevance, io.ld, io.out = RELEVANCE[relevance], ld, _ptr(out)
        self._eval_call(self.lib.vsl_highlight_pairs, io, (flat, venc, qenc, vidx, qidx, out, h_score, ws))
        return out

    def select_topm(self, key, M):
        """The best M of N per row of `key` on the device (include/vslnet_hip.h, vsl_select_topm; the written specification:
        vslnet_amd.spans.select_topm_reference) -> VideoRanks(video (G, M) int32, relevance (G, M) fp32, count (G,) int32 = min(M, N)): key descending,
        ties by the smaller index, -0.0 as +0.0.  `key`: (G, N) fp32 on the device, rows contiguous, any row stride >= N (a column slice of a wider
        matrix works).  1 <= M <= 1024."""
        self._need('video_ranking')
        M = int(M)
        _c_int('select_topm', M=M)
        if key.dim() != 2 or key.dtype != torch.float32 or not key.is_cuda or (key.shape[1] > 1 and key.stride(1) != 1):
            raise ValueError('select_topm: key must be a (G, N) cuda float32 tensor with contiguous rows, got %s %s' % (key.dtype, tuple(key.shape)))
        G, N = key.shape
        ld = int(key.stride(0)) if G > 1 else max(N, 1)
        n = max(M, 0)
        index = torch.empty(G, n, dtype=torch.int32, device=self.device)
        val = torch.empty(G, n, dtype=torch.float32, device=self.device)
        count = torch.empty(G, dtype=torch.int32, device=self.device)
        io = vsl_select_io(G, N, ld, M, key.data_ptr(), index.data_ptr(), val.data_ptr(), count.data_ptr())
        self._call(self.lib.vsl_select_topm(self.h, C.byref(io), self._stream()))
        return VideoRanks(index, val, count)

    def localize(self, flat, pad_vec, glove_vec, enc, video_index, word_ids, char_ids, q_mask):
        """Everything of forward() behind the video pass, for B queries against the resident encoding `enc`: query b is localised in video
        video_index[b].  -> (h_score, start_logits, end_logits), each (B, enc.T): the bits of forward(inference=True) on the replicated batch
        (at a T off the 32-row tile: within a few 1e-6 of it, include/vslnet_hip.h).
        `video_index` as a list / numpy array / CPU tensor is range-checked here and uploaded as int32; a DEVICE tensor (int32 or int64) is
        trusted -- no synchronising read -- and an index outside [0, enc.N) then reads outside the encoding.
        `flat` must hold the parameter values `enc` was computed with (VSLNet.localize checks that through the handle's epoch)."""
        self._need('shared_video')
        if not isinstance(enc, VideoEncoding):
            raise TypeError('localize: enc must be the VideoEncoding that encode_video returned')
        N, T = enc.N, enc.T
        B, Lq, Lc = char_ids.shape
        vidx = self._index('localize', video_index, N, 'video_index', 'the encoding holds %d videos')
        if B < 1:
            raise ValueError('localize: empty query batch')
        _chk(vidx, torch.int32, (B,), 'video_index')
        _chk(flat, torch.float32, (self.param_floats,), 'params')
        _chk(enc.encoding, torch.float32, (N, T, 128), 'encoding')
        _chk(enc.v_mask, torch.float32, (N, T), 'v_mask')
        pad_vec, glove_vec = self._check_query(B, Lq, Lc, word_ids, char_ids, q_mask, pad_vec, glove_vec)
        self._flush_loss()
        ws = self._grow_ws(self.localize_workspace_floats(B, T, Lq, Lc))
        out = self._out3(B, T)
        io = vsl_localize_io()
        io.B, io.T, io.Lq, io.Lc, io.N = B, T, Lq, Lc, N
        io.params, io.pad_vec, io.glove_vec = _ptr(flat), _ptr(pad_vec), _ptr(glove_vec)
        io.word_ids, io.char_ids, io.q_mask = _ptr(word_ids), _ptr(char_ids), _ptr(q_mask)
        io.video_encoding, io.v_mask, io.video_index = _ptr(enc.encoding), _ptr(enc.v_mask), _ptr(vidx)
        io.h_score, io.start_logits, io.end_logits = _ptr(out[0]), _ptr(out[1]), _ptr(out[2])
        io.workspace = _ptr(ws)
        self._eval_call(self.lib.vsl_localize, io, (flat, pad_vec, glove_vec, enc, vidx, word_ids, char_ids, q_mask, out, ws))
        return out[0], out[1], out[2]

    def loss(self, start_labels, end_labels, h_labels, w_loc=1.0, w_highlight=5.0, inv_batch=None, mask_sum=0.0,
             want_grads=True, scores=None, start_logits=None, end_logits=None, v_mask=None, lazy=False):
        """Fused compute_loss + compute_highlight_loss.  By default on the outputs of the LAST forward; explicit
        (B, T) tensors may be passed instead.  Returns (losses[4], d_h, d_sl, d_el).
        `lazy=True` (training steps: what `main.train` and `bench.py` do): nothing is launched here -- the loss becomes part of the next
        `backward()` on the returned seeds (vsl_io.fused_loss: for T >= 32 the loss kernel then leaves the dependent chain and the consumers of
        the seeds compute them from the logits); `losses` and the seeds are valid once that backward's work is.  Any other use of the engine
        in between (another forward / loss / a backward on other seeds) issues the pending loss first."""
        io = self._last
        if scores is not None:
            B, T, ptrs = self._check_scores(scores, start_logits, end_logits, v_mask)
            io2 = vsl_io()
            C.memmove(C.byref(io2), C.byref(io), C.sizeof(vsl_io))
            if (B, T) != (io.B, io.T):
                raise ValueError('loss inputs (%d, %d) do not match the last forward (%d, %d)' % (B, T, io.B, io.T))
            io2.h_score, io2.start_logits, io2.end_logits, io2.v_mask = ptrs
            io = io2
        B, T = io.B, io.T
        _chk(start_labels, torch.int64, (B,), 'start_labels')
        _chk(end_labels, torch.int64, (B,), 'end_labels')
        _chk(h_labels, torch.int64, (B, T), 'h_labels')
        losses = torch.empty(4, dtype=torch.float32, device=self.device)
        d = self._out3(B, T) if want_grads else None
        l = vsl_loss_io()
        l.start_labels, l.end_labels, l.h_labels = _ptr(start_labels), _ptr(end_labels), _ptr(h_labels)
        l.w_loc, l.w_highlight = float(w_loc), float(w_highlight)
        l.inv_batch = float(1.0 / B if inv_batch is None else inv_batch)
        l.mask_sum = float(mask_sum)
        l.losses = _ptr(losses)
        if want_grads:
            l.d_h_score, l.d_start_logits, l.d_end_logits = _ptr(d[0]), _ptr(d[1]), _ptr(d[2])
        self._flush_loss()
        if lazy and want_grads and scores is None and self.has_fused_io:
            self._pending_loss = (l, io, (start_labels, end_labels, h_labels, losses, d))
            return losses, d[0], d[1], d[2]
        self._call(self.lib.vsl_loss(self.h, C.byref(io), C.byref(l), self._stream()))
        return (losses,) + ((d[0], d[1], d[2]) if want_grads else (None, None, None))

    def group_loss(self, start_labels, end_labels, h_labels, group_start, positive, w_loc=1.0, w_highlight=5.0, w_rank=1.0, temperature=0.1,
                   relevance='max', inv_pos=None, inv_groups=None, mask_sum=0.0, want_grads=True, scores=None, start_logits=None, end_logits=None,
                   v_mask=None):
        """loss() over GROUPS of pair rows plus the video ranking term (include/vslnet_hip.h, vsl_group_loss; the written specification:
        vslnet_amd.spans.group_loss_reference).  By default on the outputs of the LAST forward; explicit (B, T) tensors may be passed instead.
        `group_start` (G + 1) / `positive` (G): int32 device tensors (anything else is converted and uploaded); their consistency is the caller's
        precondition.  `start_labels` / `end_labels` may be None with w_loc == 0 and `h_labels` with w_highlight == 0.  inv_pos and inv_groups
        default to 1 / G.  -> (losses[5]: loc, highlight, rank, total, mask sum used; hits: int32 scalar tensor; relevance (B,); d_h, d_sl, d_el --
        None without want_grads).  Never lazy: the call is two launches of its own, and the seeds go to backward() like any others."""
        self._need('group_loss')
        if relevance not in RELEVANCE:
            raise ValueError("group_loss: relevance must be 'max' or 'mean', got %r" % (relevance,))
        if scores is not None:
            B, T, ptrs = self._check_scores(scores, start_logits, end_logits, v_mask)
        else:
            io = self._last
            if io is None:
                raise VslError('group_loss: no forward has run and no scores were passed')
            B, T = io.B, io.T
            ptrs = (io.h_score, io.start_logits, io.end_logits, io.v_mask)
        group_start = torch.as_tensor(group_start).to(device=self.device, dtype=torch.int32).contiguous()
        positive = torch.as_tensor(positive).to(device=self.device, dtype=torch.int32).contiguous()
        G = int(positive.numel())
        _chk(group_start, torch.int32, (G + 1,), 'group_start')
        if (start_labels is None) != (end_labels is None):
            raise ValueError('group_loss: start_labels and end_labels must be both given or both None')
        if start_labels is not None:
            _chk(start_labels, torch.int64, (B,), 'start_labels')
            _chk(end_labels, torch.int64, (B,), 'end_labels')
        if h_labels is not None:
            _chk(h_labels, torch.int64, (B, T), 'h_labels')
        self._flush_loss()
        scratch = self._group_scratch.get((B, G))
        if scratch is None and 1 <= G <= B:             # (anything else: the library refuses the call by name below)
            n = C.c_int64()
            self._call(self.lib.vsl_group_loss_scratch_floats(B, G, C.byref(n)))
            scratch = self._group_scratch[(B, G)] = torch.empty(int(n.value), dtype=torch.float32, device=self.device)
        losses = torch.empty(5, dtype=torch.float32, device=self.device)
        hits = torch.empty((), dtype=torch.int32, device=self.device)
        rel = torch.empty(B, dtype=torch.float32, device=self.device)
        d = self._out3(B, T) if want_grads else None
        l = vsl_group_loss_io()
        l.B, l.T, l.G = B, T, G
        l.h_score, l.start_logits, l.end_logits, l.v_mask = ptrs
        l.start_labels, l.end_labels, l.h_labels = _ptr(start_labels), _ptr(end_labels), _ptr(h_labels)
        l.group_start, l.positive = _ptr(group_start), _ptr(positive)
        l.w_loc, l.w_highlight, l.w_rank = float(w_loc), float(w_highlight), float(w_rank)
        l.inv_pos = float(1.0 / max(G, 1) if inv_pos is None else inv_pos)
        l.inv_groups = float(1.0 / max(G, 1) if inv_groups is None else inv_groups)
        l.mask_sum = float(mask_sum)
        l.inv_temperature = float(1.0 / temperature) if temperature > 0 else 0.0
        l.relevance = RELEVANCE[relevance]
        l.losses, l.hits, l.pair_relevance, l.scratch = _ptr(losses), _ptr(hits), _ptr(rel), _ptr(scratch)
        if want_grads:
            l.d_h_score, l.d_start_logits, l.d_end_logits = _ptr(d[0]), _ptr(d[1]), _ptr(d[2])
        self._call(self.lib.vsl_group_loss(self.h, C.byref(l), self._stream()))
        return (losses, hits, rel) + ((d[0], d[1], d[2]) if want_grads else (None, None, None))

    def _flush_loss(self):
        """Issue a pending lazy loss() as its own launch (the caller did not go on to backward() on its seeds)."""
        pend, self._pending_loss = self._pending_loss, None
        if pend is not None:
            l, io, _ = pend
            self._call(self.lib.vsl_loss(self.h, C.byref(io), C.byref(l), self._stream()))

    def early_grad_offset(self):
        """First float offset of the block of `grads` that is final when `backward(..., early_event=)` fires its event."""
        return int(self.lib.vsl_early_grad_offset(self.h))

    def backward(self, d_h, d_sl, d_el, grads, early_event=None, fused_step=None, accumulate=False):
        """Backward of the LAST forward (forward() or forward_shared()); writes the flat gradient bucket `grads` (same layout as the params).
        `early_event` (torch.cuda.Event, data parallel): recorded by the library as soon as grads[early_grad_offset():] is final.
        `fused_step` (single process; `FlatAdamW.fused_step()`): dict(flat, exp_avg, exp_avg_sq, lr, step, betas, eps, weight_decay, clip_norm,
        hf_order[, grad_norm_out]) -- this optimizer step is applied inside the backward's last launch (final reduction + clip + AdamW in one
        kernel); equivalent to backward() followed by adamw_step(..., norm_from_backward=True).
        `accumulate=True` (vsl_backward_accumulate): the gradients are ADDED to what `grads` holds, one fp32 add per element behind the same sums
        (grads = grads + g).  One optimizer step over K micro-batches is the first one with accumulate=False (it overwrites: nothing is zeroed), the
        others with accumulate=True, the last of them with `fused_step`: clip and AdamW then act on the accumulated bucket and its norm.  The
        micro-batches take the global loss normalisers and their first row as forward()'s `sample_offset`, like data-parallel shards."""
        if accumulate:
            self._need('grad_accumulation')
        io = self._last
        if io is not None and io.inference:
            raise VslError('backward(): the last forward was an inference forward, which saved nothing; run forward(inference=False) on the batch')
        B, T = io.B, io.T
        pend = self._pending_loss
        fused_loss = None
        if pend is not None:
            d = pend[2][4]
            if pend[1] is io and d_h is not None and d_h.data_ptr() == d[0].data_ptr() and d_sl.data_ptr() == d[1].data_ptr() and d_el.data_ptr() == d[2].data_ptr():
                fused_loss, self._pending_loss = pend, None          # the lazy loss rides in this call
            else:
                self._flush_loss()
        if d_h is not None:
            _chk(d_h, torch.float32, (B, T), 'd_h_score')
        _chk(d_sl, torch.float32, (B, T), 'd_start_logits')
        _chk(d_el, torch.float32, (B, T), 'd_end_logits')
        _chk(grads, torch.float32, (self.param_floats,), 'grads')
        io.d_h_score, io.d_start_logits, io.d_end_logits, io.grads = _ptr(d_h), _ptr(d_sl), _ptr(d_el), _ptr(grads)
        io.early_grads_event = None
        if early_event is not None and self._last_shared is not None:
            raise ValueError('early_event belongs to the data-parallel exchange, which a shared-encoding step does not support')
        if early_event is not None:
            early_event.record(torch.cuda.current_stream(self.device))     # creates the handle lazily; harmless: recorded again by the library
            io.early_grads_event = C.c_void_p(early_event.cuda_event)
        io.fused_loss = C.cast(C.pointer(fused_loss[0]), C.c_void_p) if fused_loss is not None else None
        io.fused_step = None
        fs = None
        if fused_step is not None:
            if early_event is not None:
                raise ValueError('fused_step is the single-process step; early_event belongs to the data-parallel exchange')
            n = self.param_floats
            for nm in ('flat', 'exp_avg', 'exp_avg_sq'):
                _chk(fused_step[nm], torch.float32, (n,), nm)
            b = fused_step.get('betas', (0.9, 0.999))
            fs = vsl_fused_step()
            fs.params, fs.exp_avg, fs.exp_avg_sq = _ptr(fused_step['flat']), _ptr(fused_step['exp_avg']), _ptr(fused_step['exp_avg_sq'])
            fs.hp = vsl_adamw(float(fused_step['lr']), float(b[0]), float(b[1]), float(fused_step.get('eps', 1e-6)),
                              float(fused_step.get('weight_decay', 0.01)), float(fused_step.get('clip_norm', 1.0) or 0.0), int(fused_step['step']),
                              int(bool(fused_step.get('hf_order', False))), 1)
            gn = fused_step.get('grad_norm_out')
            fs.grad_norm_out = _ptr(gn) if gn is not None else None
            io.fused_step = C.cast(C.pointer(fs), C.c_void_p)
        stream = self._stream()
        try:
            if accumulate:
                self._call(self.lib.vsl_backward_accumulate(self.h, C.byref(io), C.byref(self._last_shared) if self._last_shared is not None else None, stream))
            elif self._last_shared is not None:
                self._call(self.lib.vsl_backward_shared(self.h, C.byref(io), C.byref(self._last_shared), stream))
            else:
                self._call(self.lib.vsl_backward(self.h, C.byref(io), stream))
        finally:
            io.fused_step = io.fused_loss = None          # (`fs` / the loss struct live until here; the library reads them during the call only)
        return grads

    def input_grads(self, out=None):
        """The gradient of the loss with respect to the video features of the LAST forward, behind its backward() (vsl_input_grads): -> fp32
        (B, T, video_feature_dim); after forward_shared (N, T, video_feature_dim), each video's gradient summed over its queries.  It is
        dropmask * (d_video_affine @ W) with the forward's own VisualProjection dropout mask: dropped features get exactly 0, padded clips their
        (non-zero) gradient.  One launch; nothing else of the step changes, and backward() launches nothing for it.  With bfloat16 features it is the
        fp32 gradient with respect to the widened features.  After backward(accumulate=True) it holds that micro-batch's rows.  `out`: a contiguous
        fp32 cuda tensor of that shape to write into.
        Raises VslError when no backward has run since the last forward, when that forward saved nothing (inference, encode_video, localize), and
        when the last backward() had `fused_step` (the weight the product needs has been updated: call backward() without it, input_grads(), then
        adamw_step(norm_from_backward=True))."""
        self._need('input_grads')
        io = self._last
        if io is None:
            raise VslError('input_grads(): no forward has run on this engine')
        if io.inference:
            raise VslError('input_grads(): the last forward was an inference forward (or encode_video / localize), which saved nothing')
        sh = self._last_shared
        shape = (sh.N if sh is not None else io.B, io.T, self.cfg.video_feature_dim)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        _chk(out, torch.float32, shape, 'out')
        self._call(self.lib.vsl_input_grads(self.h, C.byref(io), C.byref(sh) if sh is not None else None, _ptr(out), self._stream()))
        return out

    def profile_select(self, kernel):
        """Time launches of `kernel` ('*' = all, None = off) with HIP events on the launch stream."""
        self._call(self.lib.vsl_profile_select(self.h, None if kernel is None else kernel.encode()))

    def profile_read(self):
        """-> {kernel: (total_ms, launches)} since the last profile_select."""
        out, name, ms, n = {}, C.create_string_buffer(64), C.c_double(), C.c_int32()
        i = 0
        while True:
            rc = self.lib.vsl_profile_read(self.h, i, name, 64, C.byref(ms), C.byref(n))
            if rc == 2:
                break
            self._call(rc)
            out[name.value.decode()] = (ms.value, n.value)
            i += 1
        return out

    def profile_launches(self):
        """-> [dict(name, stream, start_us, stop_us, host_us, deps)] of every profiled launch since the last profile_select, in enqueue
        order (tools/critical_path.py)."""
        out, name = [], C.create_string_buffer(64)
        st, t0, t1, th, nd = C.c_int32(), C.c_double(), C.c_double(), C.c_double(), C.c_int32()
        deps = (C.c_int32 * 6)()
        i = 0
        while True:
            rc = self.lib.vsl_profile_launch(self.h, i, name, 64, C.byref(st), C.byref(t0), C.byref(t1), C.byref(th), deps, C.byref(nd))
            if rc == 2:
                break
            self._call(rc)
            out.append(dict(name=name.value.decode(), stream=st.value, start_us=t0.value, stop_us=t1.value, host_us=th.value,
                            deps=[deps[k] for k in range(nd.value)]))
            i += 1
        return out

    def adamw_step(self, flat, grads, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                   clip_norm=1.0, grad_norm_out=None, hf_order=False, norm_from_backward=False):
        """clip_grad_norm_ + AdamW on the flat buckets (main_t7.py:111-112), two kernels, no host synchronisation.
        `step` is 1-based; `grad_norm_out` (optional 1-element device tensor) receives the un-clipped global norm.
        `norm_from_backward=True`: `grads` is untouched since this engine's last backward() (single-GPU training, no exchange): the
        norm comes from the sums of squares the backward's final reduction recorded -- one kernel less."""
        n = self.param_floats
        for t, nm in ((flat, 'flat'), (grads, 'grads'), (exp_avg, 'exp_avg'), (exp_avg_sq, 'exp_avg_sq')):
            _chk(t, torch.float32, (n,), nm)
        hp = vsl_adamw(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(clip_norm or 0.0), int(step),
                       int(bool(hf_order)), int(bool(norm_from_backward)))
        self._call(self.lib.vsl_adamw_step(self.h, _ptr(flat), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), C.byref(hp),
                                           _ptr(grad_norm_out) if grad_norm_out is not None else None, self._stream()))

    def extract_index(self, start_logits, end_logits):
        B, T = start_logits.shape
        _chk(start_logits, torch.float32, (B, T), 'start_logits')
        _chk(end_logits, torch.float32, (B, T), 'end_logits')
        idx = torch.empty(2, B, dtype=torch.int64, device=self.device)
        self._call(self.lib.vsl_extract_index(self.h, _ptr(start_logits), _ptr(end_logits), B, T, _ptr(idx[0]),
                                              _ptr(idx[1]), self._stream()))
        return idx[0], idx[1]

    def extract_topk(self, start_logits, end_logits, k, nms_iou=1.0, max_span=0, lengths=None, v_mask=None, want_prob=True):
        """The k best spans per sample by greedy selection with temporal NMS (include/vslnet_hip.h, vsl_extract_topk; the written specification:
        vslnet_amd.spans.topk_spans_reference) -> TopkSpans.  Candidates are the spans inside the sample's valid length: `lengths` (B,) integers, or
        `v_mask` (B, T), a prefix mask (convert_length_to_mask) whose row sums are the lengths; neither: T.  nms_iou = 1 is plain top-k."""
        self._need('topk')
        if lengths is not None and v_mask is not None:
            raise ValueError('extract_topk: give lengths or v_mask, not both')
        B, T = start_logits.shape
        _chk(start_logits, torch.float32, (B, T), 'start_logits')
        _chk(end_logits, torch.float32, (B, T), 'end_logits')
        if v_mask is not None:
            _chk(v_mask, torch.float32, (B, T), 'v_mask')
            lengths = v_mask.sum(dim=1).to(torch.int32)
        elif lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int32).contiguous()
            _chk(lengths, torch.int32, (B,), 'lengths')
        k, max_span = int(k), int(max_span)
        _c_int('extract_topk', k=k, max_span=max_span)
        idx = torch.empty(2, B, max(k, 0), dtype=torch.int64, device=self.device)
        val = torch.empty(2 if want_prob else 1, B, max(k, 0), dtype=torch.float32, device=self.device)
        count = torch.empty(B, dtype=torch.int32, device=self.device)
        io = vsl_topk_io(start_logits.data_ptr(), end_logits.data_ptr(), lengths.data_ptr() if lengths is not None else None, B, T, k,
                         float(nms_iou), max_span, idx[0].data_ptr(), idx[1].data_ptr(), val[0].data_ptr(),
                         val[1].data_ptr() if want_prob else None, count.data_ptr())
        self._call(self.lib.vsl_extract_topk(self.h, C.byref(io), self._stream()))
        return TopkSpans(idx[0], idx[1], val[0], val[1] if want_prob else None, count)

    def merge_topk(self, spans, group_index, G, k_out, tag=None):
        """The k_out best moments of every group of top-k lists (include/vslnet_hip.h, vsl_merge_topk; the written specification:
        vslnet_amd.spans.merge_topk_reference) -> CorpusMoments.  `spans`: a TopkSpans of B lists (extract_topk(want_prob=True); the ranking key is its
        `prob`); `group_index` (B,) int32 on the device: the group (query) of list b, a value outside [0, G) drops the list; `tag`: None (list b is tagged
        b), (B,) int32 (one tag per list: its video), or (B, k) int32 (one per slot: the `tag` of an earlier merge_topk whose result is merged again --
        pass TopkSpans(m.start, m.end, m.score, m.prob, m.count) of that CorpusMoments m).  Order: prob descending, then tag, list, slot ascending."""
        self._need('merge_topk')
        B, K, G, k_out = self._check_spans('merge_topk', spans, group_index, G, k_out)
        per_slot = tag is not None and tag.dim() == 2
        if tag is not None:
            _chk(tag, torch.int32, (B, K) if per_slot else (B,), 'tag')
        n = max(G, 0), max(k_out, 0)
        i32 = torch.empty((2,) + n, dtype=torch.int32, device=self.device)
        i64 = torch.empty((2,) + n, dtype=torch.int64, device=self.device)
        f32 = torch.empty((2,) + n, dtype=torch.float32, device=self.device)
        count = torch.empty(n[0], dtype=torch.int32, device=self.device)
        io = vsl_merge_io(B, K, G, k_out, spans.start.data_ptr(), spans.end.data_ptr(), spans.score.data_ptr(), spans.prob.data_ptr(),
                          spans.count.data_ptr(), group_index.data_ptr(), tag.data_ptr() if tag is not None else None, int(per_slot),
                          i32[0].data_ptr(), i32[1].data_ptr(), i64[0].data_ptr(), i64[1].data_ptr(), f32[0].data_ptr(), f32[1].data_ptr(),
                          count.data_ptr())
        self._call(self.lib.vsl_merge_topk(self.h, C.byref(io), self._stream()))
        return CorpusMoments(i32[0], i32[1], i64[0], i64[1], f32[0], f32[1], count)


def flat_from_state_dict(engine, sd):
    """Pack a reference-style state_dict (name -> tensor) into the engine's flat parameter bucket."""
    flat = engine.new_flat()
    for n, o, k, shp in engine.layout:
        flat[o:o + k] = sd[n].reshape(-1).to(device=engine.device, dtype=torch.float32)
    return flat
