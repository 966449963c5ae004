"""Drop-in `VSLNet` module over the MI355X-native HIP path (mirror of /root/reference/model/VSLNet_t7.py:20-72).

    model = VSLNet(configs, word_vectors).to('cuda')
    h_score, start_logits, end_logits = model(word_ids, char_ids, video_features, v_mask, q_mask)
    loss = model.compute_loss(...) + 5.0 * model.compute_highlight_loss(...)
    loss.backward()

Same constructor, methods, `state_dict` keys and error behaviour as the reference; the arithmetic is ONE fused launch
sequence of hand-written gfx950 kernels reached through the C ABI (include/vslnet_hip.h).  All trainable parameters
live in one flat fp32 bucket (the nn.Parameters are views into it) and so do the gradients -- the layout data-parallel
training all-reduces as a single RCCL call (vslnet_amd/dp.py).
"""
import torch
import torch.nn as nn

from ..engine import Engine, VslError
from .layers import (Embedding, VisualProjection, FeatureEncoder, CQAttention, CQConcatenate, ConditionedPredictor,
                     HighLightLayer)


def build_optimizer_and_scheduler(model, configs):
    """VSLNet_t7.py:8-17: AdamW (no decay on bias / LayerNorm) + linear decay with warm-up.
    `transformers.AdamW` is gone from current transformers; torch.optim.AdamW with the historical HF defaults
    (eps 1e-6) is used instead -- optimizer parity is 'unpinned' (SURVEY 8c)."""
    no_decay = ('bias', 'layer_norm', 'LayerNorm')
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [{'params': [p for n, p in named if not any(k in n for k in no_decay)], 'weight_decay': 0.01},
              {'params': [p for n, p in named if any(k in n for k in no_decay)], 'weight_decay': 0.0}]
    optimizer = torch.optim.AdamW(groups, lr=configs.init_lr, eps=1e-6)
    total, warm = float(configs.num_train_steps), float(configs.num_train_steps * configs.warmup_proportion)

    def lr_lambda(step):
        if step < warm:
            return float(step) / max(1.0, warm)
        return max(0.0, (total - step) / max(1.0, total - warm))
    return optimizer, torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda)


def _feature_grad(ctx, model):
    """grad of the loss wrt the caller's `video_features` (behind the engine's backward): None unless autograd asks for it -- nothing extra is
    launched then -- otherwise Engine.input_grads() in the caller's dtype and shape.  A library without the entry point raises: a silent None
    would leave an adapter in front of the model untrained."""
    if not ctx.needs_input_grad[3]:
        return None
    eng = model._engine
    if not eng.has_input_grads:
        raise VslError('video_features requires grad, but the loaded library has no input gradients (vsl_input_grads is missing)')
    return eng.input_grads().view(ctx.vf_shape).to(ctx.vf_dtype)


class _ForwardFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, word_ids, char_ids, vfeats, v_mask, q_mask, *params):
        eng = model._engine_for(vfeats.device)
        model._step += 1
        we = model.embedding_net.word_emb
        h, sl, el = eng.forward(model._flat, we.pad_vec.data if we.is_pretrained else None,
                                we.glove_vec.data if we.is_pretrained else None, word_ids.contiguous(), char_ids.contiguous(),
                                vfeats.contiguous().float(), v_mask.contiguous().float(), q_mask.contiguous().float(),
                                training=model.training, seed=(model._seed << 20) + model._step)
        ctx.model, ctx.token = model, model._step
        ctx.vf_shape, ctx.vf_dtype = vfeats.shape, vfeats.dtype
        return h, sl, el

    @staticmethod
    def backward(ctx, d_h, d_sl, d_el):
        model = ctx.model
        if ctx.token != model._step:
            raise RuntimeError('VSLNet.backward: another forward ran since this graph was built; the HIP engine keeps the '
                               'saved activations of the latest forward only')
        # a fresh bucket per backward (autograd keeps what is returned): vsl_backward overwrites every element, so it is neither
        # zeroed nor copied
        g = model._engine.backward(d_h.contiguous(), d_sl.contiguous(), d_el.contiguous(), torch.empty_like(model._flat_grad))
        views = model._engine.views(g)
        return (None, None, None, _feature_grad(ctx, model), None, None) + tuple(views[n] for n in model._flat_names)


class _SharedForwardFn(torch.autograd.Function):
    """VSLNet.forward_shared: N videos, B queries, one encoding per video (Engine.forward_shared); the backward is the engine's own dispatch."""

    @staticmethod
    def forward(ctx, model, word_ids, char_ids, vfeats, v_mask, q_mask, video_index, *params):
        eng = model._engine_for(vfeats.device)
        model._step += 1
        we = model.embedding_net.word_emb
        vf = vfeats.contiguous()
        h, sl, el = eng.forward_shared(model._flat, we.pad_vec.data if we.is_pretrained else None, we.glove_vec.data if we.is_pretrained else None,
                                       word_ids.contiguous(), char_ids.contiguous(), vf if vf.dtype == torch.bfloat16 else vf.float(),
                                       v_mask.contiguous().float(), q_mask.contiguous().float(), video_index, training=model.training,
                                       seed=(model._seed << 20) + model._step)
        ctx.model, ctx.token = model, model._step
        ctx.vf_shape, ctx.vf_dtype = vfeats.shape, vfeats.dtype
        return h, sl, el

    @staticmethod
    def backward(ctx, d_h, d_sl, d_el):
        model = ctx.model
        if ctx.token != model._step:
            raise RuntimeError('VSLNet.backward: another forward ran since this graph was built; the HIP engine keeps the '
                               'saved activations of the latest forward only')
        g = model._engine.backward(d_h.contiguous(), d_sl.contiguous(), d_el.contiguous(), torch.empty_like(model._flat_grad))
        views = model._engine.views(g)
        return (None, None, None, _feature_grad(ctx, model), None, None, None) + tuple(views[n] for n in model._flat_names)


class _LossFn(torch.autograd.Function):
    """compute_loss / compute_highlight_loss through the fused loss kernel; `which` selects the returned term."""

    @staticmethod
    def forward(ctx, model, which, a, b, lab0, lab1, hlab, mask):
        eng = model._engine
        if which == 'loc':
            losses, d_h, d_sl, d_el = eng.loss(lab0, lab1, hlab, 1.0, 0.0, scores=a, start_logits=a, end_logits=b, v_mask=mask)
            ctx.save_for_backward(d_sl, d_el)
            return losses[0].clone()
        losses, d_h, d_sl, d_el = eng.loss(lab0, lab1, hlab, 0.0, 1.0, scores=a, start_logits=a, end_logits=a, v_mask=mask)
        ctx.save_for_backward(d_h)
        return losses[1].clone()

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        if len(saved) == 2:
            return None, None, saved[0] * g, saved[1] * g, None, None, None, None
        return None, None, saved[0] * g, None, None, None, None, None


class _RankLossFn(torch.autograd.Function):
    """compute_video_ranking_loss through the grouped loss kernels with the span and highlight weights at 0: the rank term and its seed alone."""

    @staticmethod
    def forward(ctx, model, h_score, mask, group_start, positive, temperature, relevance):
        losses, _, _, d_h, _, _ = model._engine.group_loss(None, None, None, group_start, positive, w_loc=0.0, w_highlight=0.0, w_rank=1.0,
                                                           temperature=temperature, relevance=relevance, scores=h_score, start_logits=h_score,
                                                           end_logits=h_score, v_mask=mask)
        ctx.save_for_backward(d_h)
        return losses[2].clone()

    @staticmethod
    def backward(ctx, g):
        return None, ctx.saved_tensors[0] * g, None, None, None, None, None


class VSLNet(nn.Module):
    def __init__(self, configs, word_vectors):
        super().__init__()
        self.configs = configs
        d = configs.dim
        self.embedding_net = Embedding(num_words=configs.word_size, num_chars=configs.char_size, out_dim=d,
                                       word_dim=configs.word_dim, char_dim=configs.char_dim, word_vectors=word_vectors,
                                       drop_rate=configs.drop_rate)
        self.video_affine = VisualProjection(visual_dim=configs.video_feature_dim, dim=d, drop_rate=configs.drop_rate)
        self.feature_encoder = FeatureEncoder(dim=d, num_heads=configs.num_heads, kernel_size=7, num_layers=4,
                                              max_pos_len=configs.max_pos_len, drop_rate=configs.drop_rate)
        self.cq_attention = CQAttention(dim=d, drop_rate=configs.drop_rate)
        self.cq_concat = CQConcatenate(dim=d)
        self.highlight_layer = HighLightLayer(dim=d)
        self.predictor = ConditionedPredictor(dim=d, num_heads=configs.num_heads, drop_rate=configs.drop_rate,
                                              max_pos_len=configs.max_pos_len, predictor=configs.predictor)
        self.init_parameters()
        self._engine = None
        self._flat = None
        self._flat_grad = None
        self._flat_names = None
        self._step = 0
        self._seed = int(getattr(configs, 'seed', 12345))
        self._param_epoch = 0          # bumped whenever the parameters may change (train(True), load_state_dict, a move): a VideoEncoding of an older epoch is stale

    def init_parameters(self):
        """VSLNet_t7.py:42-50: Xavier-uniform conv/linear weights, zero biases, nn.LSTM.reset_parameters() for the rnn head.
        Same module order and the same initialisers as the reference, so the same torch seed gives bit-identical weights
        (pinned by tests/test_oracle_golden.py::test_init_matches_reference_under_the_same_seed)."""
        def init_weights(m):
            if isinstance(m, (nn.Conv2d, nn.Conv1d, nn.Linear)):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LSTM):
                m.reset_parameters()
        self.apply(init_weights)

    # ---- flat parameter bucket ------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._engine = None            # device / dtype may have changed: rebuild lazily
        self._flat = None
        self._param_epoch = getattr(self, '_param_epoch', 0) + 1
        return out

    def train(self, mode=True):
        if mode:
            self._param_epoch += 1     # training may update the parameters: encodings computed before it are stale
        return super().train(mode)

    def load_state_dict(self, *a, **k):
        self._param_epoch += 1
        return super().load_state_dict(*a, **k)

    def _engine_for(self, device):
        if self._engine is not None and self._flat is not None:
            return self._engine
        pdev = next(self.parameters()).device
        if pdev.type != 'cuda':
            raise RuntimeError('VSLNet (vslnet_amd) runs on an MI355X only: move the module with .to("cuda") first; there is '
                               'no CPU fallback')
        eng = Engine(self.configs, device=pdev, word_table=not self.embedding_net.word_emb.is_pretrained)
        named = dict(self.named_parameters())
        flat = eng.new_flat()
        for n, o, k, shp in eng.layout:
            p = named[n]
            if tuple(p.shape) != tuple(shp):
                raise RuntimeError('parameter %s has shape %s, engine expects %s' % (n, tuple(p.shape), shp))
            flat[o:o + k].view(shp).copy_(p.data)
            p.data = flat[o:o + k].view(shp)       # the nn.Parameter now aliases the flat bucket
        self._engine, self._flat = eng, flat
        self._flat_grad = eng.new_flat()
        self._flat_names = [n for n, _, _, _ in eng.layout]
        self._flat_params = [named[n] for n in self._flat_names]
        return eng

    @property
    def flat_parameters(self):
        """(flat params, flat grads) buckets -- what the data-parallel wrapper all-reduces / the fused optimizer walks."""
        self._engine_for(None)
        return self._flat, self._flat_grad

    def state_dict_from_flat(self, host_flat):
        """`self.state_dict()` (same keys, order, shapes) with the trainable entries taken from a HOST copy of the flat bucket and the
        frozen ones (pad_vec, glove_vec) from a host copy made once -- the checkpoint writer's path (runner.CheckpointWriter.save_flat)."""
        from collections import OrderedDict
        eng = self._engine_for(None)
        views = {n: host_flat[o:o + k].view(shp) for n, o, k, shp in eng.layout}
        if getattr(self, '_frozen_host', None) is None:
            self._frozen_host = {k: v.detach().cpu() for k, v in self.state_dict().items() if k not in views}
        return OrderedDict((k, views[k] if k in views else self._frozen_host[k]) for k in self.state_dict().keys())

    # ---- reference API ---------------------------------------------------------------------------------------------
    def forward(self, word_ids, char_ids, video_features, v_mask, q_mask):
        eng = self._engine_for(video_features.device)
        if not self.training and not torch.is_grad_enabled() and eng.has_inference and eng.use_inference:
            # evaluation that will never be differentiated (runner.eval_test, main.py --mode test): the inference path -- kernels that save
            # nothing and the forward-only workspace plan; same bits as the saved path.  eval() WITH grad enabled keeps the saved path (a
            # backward may follow); a library without the mode (an A/B baseline) falls back to it as well
            self._step += 1                                 # (a graph built on an earlier forward is stale: its saves are overwritten)
            we = self.embedding_net.word_emb
            return eng.forward(self._flat, we.pad_vec.data if we.is_pretrained else None, we.glove_vec.data if we.is_pretrained else None,
                               word_ids.contiguous(), char_ids.contiguous(), video_features.contiguous().float(), v_mask.contiguous().float(),
                               q_mask.contiguous().float(), inference=True)
        return _ForwardFn.apply(self, word_ids, char_ids, video_features, v_mask, q_mask, *self._flat_params)

    # ---- training through a shared video encoding (no reference counterpart: the reference runs the video half once per sample) ----
    def forward_shared(self, word_ids, char_ids, video_features, v_mask, q_mask, video_index):
        """forward() over N videos and B queries: `video_features` (N, T, video_feature_dim) and `v_mask` (N, T) per VIDEO, the query tensors per
        query, query b paired with video video_index[b] (list / numpy / CPU tensor: range-checked; device tensor: trusted).  VisualProjection and
        the video pass of the feature encoder run once per video, forward and backward; -> (h_score, start_logits, end_logits), each (B, T), for
        compute_loss / compute_highlight_loss (with the per-query mask v_mask[video_index]) and .backward().  The video half's dropout draws one
        mask per video: at drop_rate 0 this is forward() on the replicated batch, otherwise a different, equally valid stochastic estimate
        (DESIGN section 7).  A training / grad-enabled call: evaluation that is never differentiated goes through encode_video + localize."""
        if not self.training and not torch.is_grad_enabled():
            raise RuntimeError('VSLNet.forward_shared is the training step through a shared encoding; under eval() + no_grad() use encode_video + localize')
        self._engine_for(video_features.device)
        return _SharedForwardFn.apply(self, word_ids, char_ids, video_features, v_mask, q_mask, video_index, *self._flat_params)

    # ---- one encoding per video, many queries against it (no reference counterpart: the reference encodes the video once per query) ----
    def _shared_video_mode(self, what):
        if self.training or torch.is_grad_enabled():
            raise RuntimeError('VSLNet.%s is evaluation only (nothing is saved for a backward): call it under model.eval() and torch.no_grad()%s'
                               % (what, ' -- the module is in train mode' if self.training else ' -- grad is enabled'))

    def encode_video(self, video_features, v_mask):
        """VisualProjection + the shared feature encoder over N videos, once: -> VideoEncoding for `localize`.  (N, T, video_feature_dim)
        features (fp32, or bfloat16 for the bf16 throughput mode) and the (N, T) clip mask.  The handle belongs to this module, this T and
        the parameters as they are now: `train()`, `load_state_dict` or moving the module make it stale."""
        self._shared_video_mode('encode_video')
        eng = self._engine_for(video_features.device)
        vf = video_features.contiguous()
        enc = eng.encode_video(self._flat, vf if vf.dtype == torch.bfloat16 else vf.float(), v_mask.contiguous().float())
        enc.owner, enc.epoch = self, self._param_epoch
        return enc

    def localize(self, enc, video_index, word_ids, char_ids, q_mask, T=None):
        """forward() for B queries against videos that `encode_video` has already encoded: query b is localised in video video_index[b].
        -> (h_score, start_logits, end_logits), each (B, enc.T): what forward(word_ids, char_ids, features[video_index], v_mask[video_index], q_mask)
        returns under eval() + no_grad() -- bit for bit at T % 32 == 0 or T <= 32, within a few 1e-6 at other T.  `T` (optional): the padded length the caller expects; an encoding of
        another T is refused (an encoding belongs to its T: the same video padded to another length encodes differently).
        `video_index`: list / numpy / CPU tensor (range-checked) or a device tensor (trusted)."""
        self._shared_video_mode('localize')
        if getattr(enc, 'owner', None) is not self:
            raise ValueError('VSLNet.localize: this VideoEncoding was made by another module (or not by VSLNet.encode_video)')
        if enc.epoch != self._param_epoch:
            raise ValueError('VSLNet.localize: stale VideoEncoding -- the parameters may have changed since it was computed (train(), load_state_dict '
                             'or a move ran in between): call encode_video again')
        if T is not None and int(T) != enc.T:
            raise ValueError('VSLNet.localize: the encoding was computed at T=%d, not T=%d: an encoding belongs to its padded T, encode again at that T' % (enc.T, int(T)))
        eng = self._engine_for(enc.encoding.device)
        self._step += 1                                     # (a graph built on an earlier forward is stale: its saves are overwritten)
        we = self.embedding_net.word_emb
        return eng.localize(self._flat, we.pad_vec.data if we.is_pretrained else None, we.glove_vec.data if we.is_pretrained else None, enc,
                            video_index, word_ids.contiguous(), char_ids.contiguous(), q_mask.contiguous().float())

    # ---- one encoding per query, pairs of resident encodings, a search over the videos of an encoding (no reference counterpart) ----
    def encode_query(self, word_ids, char_ids, q_mask):
        """The embedding and the query pass of the shared feature encoder over Q queries, once: -> QueryEncoding for `localize_pairs` / `retrieve`.
        The handle belongs to this module, this Lq / Lc and the parameters as they are now: `train()`, `load_state_dict` or moving the module make it
        stale."""
        self._shared_video_mode('encode_query')
        eng = self._engine_for(char_ids.device)
        we = self.embedding_net.word_emb
        enc = eng.encode_query(self._flat, we.pad_vec.data if we.is_pretrained else None, we.glove_vec.data if we.is_pretrained else None,
                               word_ids.contiguous(), char_ids.contiguous(), q_mask.contiguous().float())
        enc.owner, enc.epoch = self, self._param_epoch
        return enc

    def _check_handle(self, enc, what, kind):
        if getattr(enc, 'owner', None) is not self:
            raise ValueError('VSLNet.%s: this %s was made by another module (or not by this module\'s encode call)' % (what, kind))
        if enc.epoch != self._param_epoch:
            raise ValueError('VSLNet.%s: stale %s -- the parameters may have changed since it was computed (train(), load_state_dict or a move ran '
                             'in between): encode again' % (what, kind))

    def localize_pairs(self, venc, qenc, video_index, query_index):
        """localize() for pairs of resident encodings: pair b is query query_index[b] of `qenc` (encode_query) in video video_index[b] of `venc`
        (encode_video).  -> (h_score, start_logits, end_logits), each (B, venc.T).  No query is embedded or encoded here.  Indices: list / numpy / CPU
        tensor (range-checked) or a device tensor (trusted)."""
        self._shared_video_mode('localize_pairs')
        self._check_handle(venc, 'localize_pairs', 'VideoEncoding')
        self._check_handle(qenc, 'localize_pairs', 'QueryEncoding')
        eng = self._engine_for(venc.encoding.device)
        self._step += 1                                     # (a graph built on an earlier forward is stale: its saves are overwritten)
        return eng.localize_pairs(self._flat, venc, qenc, video_index, query_index)

    def merge_topk(self, spans, group_index, G, k_out, tag=None):
        """The k_out best moments of every group of top-k lists (Engine.merge_topk) -> CorpusMoments(tag, list, start, end, score, prob, count)."""
        self._engine_for(spans.start.device)
        return self._engine.merge_topk(spans, group_index, G, k_out, tag=tag)

    def rank_videos(self, venc, qenc, m, relevance='max', pairs_per_call=4096):
        """The m most relevant videos of `venc` for every query of `qenc` -> VideoRanks(video (Q, m) int32, relevance (Q, m) float32, count (Q,) int32 =
        min(m, N)), ranked: relevance descending, ties by the smaller video number; slots from count on hold -1, 0.  The relevance of a (query, video)
        pair is the 'max' or the 'mean' of its query-guided highlight score over the video's valid clips (-inf for a video without one): the
        forward up to the highlight layer, no predictor.  Every query runs against every video in the chunks `retrieve` uses -- all queries x a block
        of videos, at most `pairs_per_call` pairs -- through highlight_pairs straight into one (Q, N) matrix; one select_topm ranks it.  1 <= m <= 1024.
        A WindowEncoding is taken as the VideoEncoding it is: its "videos" are its windows.  Nothing goes through the host."""
        self._shared_video_mode('rank_videos')
        self._check_handle(venc, 'rank_videos', 'VideoEncoding')
        self._check_handle(qenc, 'rank_videos', 'QueryEncoding')
        return self._rank_videos(venc, qenc, m, relevance, pairs_per_call, 'rank_videos')

    def _rank_videos(self, venc, qenc, m, relevance, pairs_per_call, what):
        Q, N, dev = qenc.Q, venc.N, venc.encoding.device
        if pairs_per_call < Q:
            raise ValueError('%s: pairs_per_call=%d is less than one video for each of the %d queries' % (what, pairs_per_call, Q))
        eng = self._engine_for(dev)
        per = max(1, pairs_per_call // Q)                    # videos per chunk
        queries = torch.arange(Q, dtype=torch.int32, device=dev)
        matrix = torch.empty(Q, N, dtype=torch.float32, device=dev)
        for v0 in range(0, N, per):
            nv = min(per, N - v0)
            qidx = queries.repeat_interleave(nv)            # pair (q, v) at q * nv + (v - v0), as in retrieve
            vidx = torch.arange(v0, v0 + nv, dtype=torch.int32, device=dev).repeat(Q)
            self._step += 1                                 # (a graph built on an earlier forward is stale: its saves are overwritten)
            eng.highlight_pairs(self._flat, venc, qenc, vidx, qidx, relevance=relevance, out=matrix, ld=N)
        return eng.select_topm(matrix, m)

    def retrieve(self, venc, qenc, k, nms_iou=0.5, max_span=0, lengths=None, pairs_per_call=4096, prefilter=0, relevance='max', return_ranks=False):
        """The k best moments of every query of `qenc` over ALL videos of `venc` -> CorpusMoments shaped (Q, k): `tag` = the video (its number in
        `venc`), start / end = the clips in that video, `prob` = the ranking key, descending; ties by video, then by the per-video rank.
        Every query runs against every video in chunks of at most `pairs_per_call` pairs -- all queries x a block of videos: localize_pairs,
        extract_topk(k, nms_iou, max_span, want_prob=True) per pair, merge_topk per query -- and one second merge_topk joins the chunks.  NMS acts
        inside a video.  `lengths` (N,): valid clips per video (default: the row sums of venc.v_mask).  Nothing goes through the host.
        `prefilter` = M >= 1 (coarse to fine): rank_videos(m = min(M, 1024), relevance) first, then the steps above over the Q min(M, N) selected
        (query, video) pairs only, in chunks of `pairs_per_call` pairs.  A moment in a video the first stage did not select cannot be returned: the
        result is that of the exhaustive search restricted to the selected pairs -- the exhaustive result itself, field by field, when M >= N.  `list`
        then numbers the rows as the exhaustive search with this `pairs_per_call` numbers them.  M > 1024 means "all videos" when N <= 1024 and is
        refused otherwise.  prefilter = 0: no first stage, the exhaustive search.  `return_ranks` (with prefilter): -> (CorpusMoments, the first stage's
        VideoRanks)."""
        from ..engine import TopkSpans, TOPM_MAX_M
        self._shared_video_mode('retrieve')
        self._check_handle(venc, 'retrieve', 'VideoEncoding')
        self._check_handle(qenc, 'retrieve', 'QueryEncoding')
        Q, N, dev = qenc.Q, venc.N, venc.encoding.device
        if pairs_per_call < Q:
            raise ValueError('retrieve: pairs_per_call=%d is less than one video for each of the %d queries' % (pairs_per_call, Q))
        prefilter = int(prefilter)
        if prefilter < 0:
            raise ValueError('retrieve: prefilter=%d must be 0 (exhaustive) or the number of videos to keep per query' % prefilter)
        if prefilter > TOPM_MAX_M and N > TOPM_MAX_M:
            raise ValueError('retrieve: prefilter=%d with N=%d videos: the first stage selects at most %d videos per query' % (prefilter, N, TOPM_MAX_M))
        if prefilter and not self._engine_for(dev).has_video_ranking:
            raise VslError('retrieve: prefilter needs a library that can rank videos (vsl_highlight_pairs / vsl_select_topm are missing)')
        lengths = (venc.v_mask.sum(dim=1) if lengths is None else torch.as_tensor(lengths, device=dev)).to(torch.int32)
        per = max(1, pairs_per_call // Q)                    # videos per chunk
        queries = torch.arange(Q, dtype=torch.int32, device=dev)
        first, ranks = [], None
        if prefilter:
            ranks = self._rank_videos(venc, qenc, min(prefilter, TOPM_MAX_M), relevance, pairs_per_call, 'retrieve')
            m = min(prefilter, N)                           # every query has exactly m selected videos
            vall = ranks.video[:, :m].reshape(-1)           # pair (q, rank r) at q * m + r
            qall = queries.repeat_interleave(m)
            for p0 in range(0, Q * m, pairs_per_call):
                vidx, qidx = vall[p0:p0 + pairs_per_call].contiguous(), qall[p0:p0 + pairs_per_call].contiguous()
                _, sl, el = self.localize_pairs(venc, qenc, vidx, qidx)
                spans = self.extract_topk(sl, el, k, nms_iou=nms_iou, max_span=max_span, lengths=lengths[vidx.long()], want_prob=True)
                first.append(self.merge_topk(spans, qidx, Q, k, tag=vidx))
        else:
            for v0 in range(0, N, per):
                nv = min(per, N - v0)
                qidx = queries.repeat_interleave(nv)            # pair (q, v) at q * nv + (v - v0)
                vidx = torch.arange(v0, v0 + nv, dtype=torch.int32, device=dev).repeat(Q)
                _, sl, el = self.localize_pairs(venc, qenc, vidx, qidx)
                spans = self.extract_topk(sl, el, k, nms_iou=nms_iou, max_span=max_span, lengths=lengths[vidx.long()], want_prob=True)
                first.append(self.merge_topk(spans, qidx, Q, k, tag=vidx))
        if len(first) == 1:
            out = first[0]
        else:
            cat = lambda name: torch.cat([getattr(m, name) for m in first]).contiguous()      # noqa: E731
            out = self.merge_topk(TopkSpans(cat('start'), cat('end'), cat('score'), cat('prob'), cat('count')), queries.repeat(len(first)), Q, k, tag=cat('tag'))
        if prefilter:
            # `list` as the exhaustive search reports it: the pair's row q * N + video of its single call, or row chunk * Q + q of its second merge
            q = queries.unsqueeze(1)
            row = q * N + out.tag if N <= per else torch.div(out.tag, per, rounding_mode='floor') * Q + q
            out = out._replace(list=torch.where(out.tag >= 0, row, out.tag).to(torch.int32))
        return (out, ranks) if return_ranks else out

    # ---- videos of any length: sliding windows, one ranked list of moments per (video, query) in the video's own clips (no reference counterpart) ----
    def encode_windows(self, videos, window, stride, windows_per_call=256):
        """The sliding windows of one or several videos of ANY length through VisualProjection and the shared feature encoder -> WindowEncoding, a
        VideoEncoding over all windows (T = `window`) for `localize_long` (and `localize` / `localize_pairs`).  `videos`: one (L, video_feature_dim)
        tensor or a list of them, fp32 or bfloat16 (the bf16 throughput mode), each of its own length.  Window w of a video starts at clip w * stride;
        a video has one window when L <= window, else ceil((L - window) / stride) + 1, the last one possibly short (spans.window_table).  Each clip
        is projected once however many windows hold it and the (windows, window, video_feature_dim) block is never built.  The library runs in
        chunks of at most `windows_per_call` windows, each handed only the feature rows its windows span (one video: a view; several: their
        concatenation), so the row limits apply per chunk; the result does not depend on the chunking where the encoder's output does not depend on
        a sample's position in its batch (window % 32 == 0 or window <= 32: exactly; elsewhere within a few 1e-6)."""
        import numpy as np
        from ..engine import WindowEncoding
        from ..spans import window_table
        self._shared_video_mode('encode_windows')
        videos = [videos] if torch.is_tensor(videos) else list(videos)
        window, stride, per = int(window), int(stride), int(windows_per_call)
        if not videos:
            raise ValueError('encode_windows: no video')
        if stride < 1:
            raise ValueError('encode_windows: stride=%d must be at least 1' % stride)
        if stride > window:
            raise ValueError('encode_windows: stride=%d > window=%d: clips between two windows would be skipped' % (stride, window))
        if window > self.configs.max_pos_len:
            raise ValueError('encode_windows: window=%d > max_pos_len=%d: the model has no positional row for such a window' % (window, self.configs.max_pos_len))
        if per < 1:
            raise ValueError('encode_windows: windows_per_call=%d must be at least 1' % per)
        bf16 = videos[0].dtype == torch.bfloat16
        for v in videos:
            if v.dim() != 2 or v.shape[0] < 1 or (v.dtype == torch.bfloat16) != bf16:
                raise ValueError('encode_windows: every video must be a (L >= 1, video_feature_dim) tensor and all of one precision, got %s %s' % (tuple(v.shape), v.dtype))
        eng = self._engine_for(videos[0].device)
        if not eng.has_windows:
            raise VslError('the loaded library has no sliding windows (vsl_encode_windows / vsl_merge_windows are missing)')
        videos = [v.contiguous() if bf16 else v.contiguous().float() for v in videos]
        lengths = np.array([int(v.shape[0]) for v in videos], dtype=np.int64)
        tabs = [window_table(L, window, stride) for L in lengths]
        first = np.concatenate([[0], np.cumsum([len(t[0]) for t in tabs])]).astype(np.int64)
        video_of = np.concatenate([np.full(len(t[0]), i, dtype=np.int64) for i, t in enumerate(tabs)])
        offset, wlen = np.concatenate([t[0] for t in tabs]), np.concatenate([t[1] for t in tabs])
        N, dev = int(first[-1]), eng.device
        enc = torch.empty(N, window, 128, dtype=torch.float32, device=dev)
        mask = torch.empty(N, window, dtype=torch.float32, device=dev)
        wrow = np.zeros(N, dtype=np.int64)
        calls = []
        for a in range(0, N, per):                          # the feature rows of a chunk: for each of its videos, the clips its windows span
            b, parts, base = min(N, a + per), [], 0
            for v in range(int(video_of[a]), int(video_of[b - 1]) + 1):
                w = np.arange(max(a, first[v]), min(b, first[v + 1]))
                lo, hi = int(offset[w[0]]), int(offset[w[-1]] + wlen[w[-1]])
                wrow[w] = base + offset[w] - lo
                parts.append(videos[v][lo:hi])
                base += hi - lo
            calls.append((a, b, parts))
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)      # noqa: E731
        d_row, d_len = up(wrow), up(wlen)
        for a, b, parts in calls:
            eng.encode_windows(self._flat, parts[0] if len(parts) == 1 else torch.cat(parts), d_row[a:b], d_len[a:b], window, out=enc[a:b], out_mask=mask[a:b])
        return WindowEncoding(enc, mask, up(video_of), up(offset), d_len, lengths, first, window, stride, owner=self, epoch=self._param_epoch)

    def localize_long(self, wenc, qenc, k, nms_iou=0.5, max_span=0, pairs=None, pairs_per_call=4096):
        """The k best moments of (video, query) pairs over videos of any length, in each video's OWN clip indices -> LongMoments(window, start, end,
        score, prob, count) shaped (P, k).  `wenc`: the WindowEncoding of encode_windows, `qenc`: a QueryEncoding.  By default every query of `qenc`
        runs against every video of `wenc` (pair p = video * Q + query); `pairs`: (P, 2) integers as (video, query).  Every window of a pair's video
        is localised against the query (localize_pairs in chunks of at most `pairs_per_call` (window, query) lists), extract_topk(k, nms_iou,
        max_span) with the window's own length leaves k moments per window at window-local indices, and ONE merge_windows -- a group per pair, ranked
        by `prob` -- shifts them to the video's clips and suppresses across the windows with the same nms_iou: a moment two overlapping windows
        report is written once.  `window` is the row of `wenc` a moment came from.  Nothing goes through the host."""
        import numpy as np
        from ..engine import LongMoments, TopkSpans, WindowEncoding
        self._shared_video_mode('localize_long')
        if not isinstance(wenc, WindowEncoding):
            raise TypeError('localize_long: wenc must be the WindowEncoding that encode_windows returned')
        self._check_handle(wenc, 'localize_long', 'WindowEncoding')
        self._check_handle(qenc, 'localize_long', 'QueryEncoding')
        V, Q, dev, k = len(wenc.lengths), qenc.Q, wenc.encoding.device, int(k)
        if pairs is None:
            pv, pq = np.repeat(np.arange(V, dtype=np.int64), Q), np.tile(np.arange(Q, dtype=np.int64), V)
        else:
            pairs = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs, dtype=np.int64).reshape(-1, 2)
            pv, pq = pairs[:, 0], pairs[:, 1]
            if len(pv) == 0 or pv.min() < 0 or pv.max() >= V or pq.min() < 0 or pq.max() >= Q:
                raise ValueError('localize_long: pairs must be (P >= 1, 2) rows of (video in [0, %d), query in [0, %d))' % (V, Q))
        if int(pairs_per_call) < 1:
            raise ValueError('localize_long: pairs_per_call=%d must be at least 1' % int(pairs_per_call))
        nwin = (wenc.first_window[1:] - wenc.first_window[:-1])[pv]               # lists of each pair: one per window of its video
        group = np.repeat(np.arange(len(pv), dtype=np.int64), nwin)
        widx = np.concatenate([np.arange(wenc.first_window[v], wenc.first_window[v + 1]) for v in pv])
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)      # noqa: E731
        d_w, d_q, d_g = up(widx), up(pq[group]), up(group)
        B = len(widx)
        idx = torch.empty(2, B, max(k, 0), dtype=torch.int64, device=dev)
        val = torch.empty(2, B, max(k, 0), dtype=torch.float32, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        d_len = wenc.window_len[d_w.long()]
        for a in range(0, B, int(pairs_per_call)):
            b = min(B, a + int(pairs_per_call))
            _, sl, el = self.localize_pairs(wenc, qenc, d_w[a:b], d_q[a:b])
            s = self.extract_topk(sl, el, k, nms_iou=nms_iou, max_span=max_span, lengths=d_len[a:b], want_prob=True)
            idx[0, a:b], idx[1, a:b], val[0, a:b], val[1, a:b], count[a:b] = s.start, s.end, s.score, s.prob, s.count
        m = self._engine.merge_windows(TopkSpans(idx[0], idx[1], val[0], val[1], count), d_g, len(pv), k, offset=wenc.offset_of_window[d_w.long()].contiguous(),
                                       nms_iou=nms_iou)
        window = torch.where(m.list >= 0, d_w[m.list.clamp(min=0).long()], m.list)
        return LongMoments(window, m.start, m.end, m.score, m.prob, m.count)

    def extract_index(self, start_logits, end_logits):
        self._engine_for(start_logits.device)
        return self._engine.extract_index(start_logits.detach().contiguous(), end_logits.detach().contiguous())

    def extract_topk(self, start_logits, end_logits, k, nms_iou=1.0, max_span=0, lengths=None, v_mask=None, want_prob=True):
        """The k best moments per query with temporal NMS (Engine.extract_topk) -> TopkSpans(start, end, score, prob, count); no reference counterpart."""
        self._engine_for(start_logits.device)
        return self._engine.extract_topk(start_logits.detach().contiguous(), end_logits.detach().contiguous(), k, nms_iou=nms_iou, max_span=max_span,
                                         lengths=lengths, v_mask=None if v_mask is None else v_mask.detach().contiguous().float(), want_prob=want_prob)

    def compute_highlight_loss(self, scores, labels, mask):
        B = scores.shape[0]
        z = torch.zeros(B, dtype=torch.int64, device=scores.device)
        return _LossFn.apply(self, 'hl', scores.contiguous(), None, z, z, labels.contiguous().long(), mask.contiguous().float())

    def compute_video_ranking_loss(self, h_score, v_mask, group_start, positive, temperature=0.1, relevance='max'):
        """The video ranking term of Engine.group_loss (include/vslnet_hip.h, vsl_group_loss; no reference counterpart): the B rows of `h_score` are G
        contiguous groups (group_start (G + 1), positive (G)), each one query against several videos with its own video at row positive[g]; the
        loss is the mean over the groups of -log softmax(relevance / temperature)[positive], the relevance being the 'max' / 'mean' of h_score over
        the valid clips that rank_videos ranks by.  Differentiable with respect to h_score: loc + a * hl + b * rank works in eager mode."""
        self._engine_for(h_score.device)
        return _RankLossFn.apply(self, h_score.contiguous().float(), v_mask.contiguous().float(), group_start, positive, float(temperature), relevance)

    def compute_loss(self, start_logits, end_logits, start_labels, end_labels):
        B, T = start_logits.shape
        zh = torch.zeros(B, T, dtype=torch.int64, device=start_logits.device)
        ones = torch.ones(B, T, dtype=torch.float32, device=start_logits.device)
        return _LossFn.apply(self, 'loc', start_logits.contiguous(), end_logits.contiguous(), start_labels.contiguous().long(),
                             end_labels.contiguous().long(), zh, ones)
