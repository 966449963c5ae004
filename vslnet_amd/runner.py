"""Evaluation loop, metrics and checkpoint housekeeping of the VSLNet path.

Mirrors `util/runner_utils_t7.py`: set_th_config :11-18, checkpoint helpers :21-45, convert_length_to_mask :48-52, IoU
metrics :55-68, eval_test :71-101.  Span extraction runs in the library's scan kernel (`VSLNet.extract_index` ->
vsl_extract_index), the metrics are host arithmetic on a few floats per sample."""
import glob
import os
import random

import numpy as np
import torch

from .data import index_to_time
from .spans import TopK, spans_to_times           # noqa: F401  (TopK re-exported: the `topk` argument of eval_test / eval_test_shared)
from .synthetic import convert_length_to_mask     # noqa: F401  (re-exported: runner_utils_t7.py:48-52)


def set_th_config(seed):
    """runner_utils_t7.py:11-18 (the cudnn switches have no ROCm meaning and are left alone)."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def _step_of(path, suffix):
    return int(os.path.basename(path).split('_')[1][:-(len(suffix) + 1)])


def filter_checkpoints(model_dir, suffix='t7', max_to_keep=5):
    """runner_utils_t7.py:21-32: keep the max_to_keep checkpoints with the highest step in `<name>_<step>.<suffix>`."""
    paths = sorted(glob.glob(os.path.join(model_dir, '*.{}'.format(suffix))), key=lambda p: _step_of(p, suffix))
    for p in paths[:max(0, len(paths) - max_to_keep)]:
        os.remove(p)


class _LazyState:
    """state_dict of a flat-bucket module from a host copy of the bucket (built on the worker thread)."""

    def __init__(self, model, host_flat, free=None):
        self.model, self.host, self.free = model, host_flat, free

    def build(self):
        try:
            return self.model.state_dict_from_flat(self.host.clone())    # a private copy ...
        finally:
            if self.free is not None:
                self.free.set()                                          # ... after which the pinned buffer may be reused (save_flat waits for this)


class CheckpointWriter:
    """`torch.save(model.state_dict(), path)` + `filter_checkpoints` (main_t7.py:125-126) off the training loop: the state is copied to
    pinned host memory on a side stream (the step's kernels keep running), a worker thread writes the file and prunes old ones.
    The reference saves whenever r1i7 >= the best so far, i.e. at every evaluation while the metric ties; a synchronous save costs
    ~14 ms (D2H of the state, pickle, file write) = 15 training steps at the headline shape (tools/e2e_rate.py)."""

    def __init__(self, device):
        import queue
        import threading
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == 'cuda' else None
        self.q = queue.Queue()
        self.err = None
        self.thread = threading.Thread(target=self._work, daemon=True)
        self.thread.start()

    def _work(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            state, event, path, model_dir, suffix, keep = item
            try:
                if event is not None:
                    event.synchronize()
                if isinstance(state, _LazyState):
                    state = state.build()
                tmp = path + '.tmp'                      # a crash / Ctrl-C mid-write must not leave a truncated *.t7 for get_last_checkpoint
                torch.save(state, tmp)
                os.replace(tmp, path)
                filter_checkpoints(model_dir, suffix=suffix, max_to_keep=keep)
            except Exception as e:                       # raised by the next save() / save_flat() / close()
                self.err = e
                if isinstance(state, _LazyState) and state.free is not None:
                    state.free.set()

    def _raise_pending(self):
        """A failed write stops the run at the next save, like the reference's synchronous torch.save would (main_t7.py:125)."""
        if self.err is not None:
            err, self.err = self.err, None
            raise err

    def save(self, state_dict, path, model_dir, suffix='t7', max_to_keep=3):
        self._raise_pending()
        if self.stream is None:
            self.q.put(({k: v.clone() for k, v in state_dict.items()}, None, path, model_dir, suffix, max_to_keep))
            return
        self.stream.wait_stream(torch.cuda.current_stream(self.device))          # the values as of this point of the training stream
        with torch.cuda.stream(self.stream):
            host = {}
            for k, v in state_dict.items():
                h = torch.empty(v.shape, dtype=v.dtype, device='cpu', pin_memory=True)
                h.copy_(v, non_blocking=True)
                host[k] = h
            ev = torch.cuda.Event()
            ev.record(self.stream)
        # the optimizer must not overwrite the parameters before the copies have read them
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        self.q.put((host, ev, path, model_dir, suffix, max_to_keep))

    def save_flat(self, model, path, model_dir, suffix='t7', max_to_keep=3):
        """The same for a module whose trainable parameters live in ONE flat bucket (vslnet_amd.model.VSLNet): a device-side snapshot of the
        bucket on the training stream (4.4 MB, microseconds; the optimizer may go on at once), ONE device-to-host copy of it on the side
        stream, and the worker thread rebuilds the reference's state_dict (same keys, shapes, order) from views of the host copy.  The
        per-tensor path above costs ~110 small copies the training stream has to wait for (3.4 ms per checkpoint)."""
        import threading
        self._raise_pending()
        flat, _ = model.flat_parameters
        snap = flat.clone()
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        if getattr(self, '_pin', None) is None or self._pin[0].numel() != snap.numel():
            self._pin = [torch.empty(snap.shape, dtype=snap.dtype, device='cpu', pin_memory=True) for _ in range(2)]
            self._pin_free = [threading.Event(), threading.Event()]
            for e in self._pin_free:
                e.set()
            self._pin_i = 0
        self._pin_i ^= 1
        # two buffers: the worker may still be writing the previous checkpoint.  Back-pressure: a buffer is reused only after the worker
        # has taken its private copy of it (blocks only when the writer lags two saves behind -- a slow disk, tiny epochs)
        free = self._pin_free[self._pin_i]
        free.wait()
        self._raise_pending()
        free.clear()
        with torch.cuda.stream(self.stream):
            host = self._pin[self._pin_i]
            host.copy_(snap, non_blocking=True)
            snap.record_stream(self.stream)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.q.put((_LazyState(model, host, free), ev, path, model_dir, suffix, max_to_keep))

    def close(self):
        self.q.put(None)
        self.thread.join()
        self._raise_pending()


def get_last_checkpoint(model_dir, suffix='t7'):
    """runner_utils_t7.py:35-45."""
    paths = glob.glob(os.path.join(model_dir, '*.{}'.format(suffix)))
    if not paths:
        raise ValueError('no *.%s checkpoint in %s' % (suffix, model_dir))
    return max(paths, key=lambda p: _step_of(p, suffix))


def calculate_iou(i0, i1):
    """runner_utils_t7.py:64-68: temporal IoU of two [start, end] intervals (hull as the union), floored at 0."""
    hull = max(i0[1], i1[1]) - min(i0[0], i1[0])
    inter = min(i0[1], i1[1]) - max(i0[0], i1[0])
    return max(0.0, 1.0 * inter / hull)


def calculate_iou_accuracy(ious, threshold):
    """runner_utils_t7.py:55-61: percentage of samples with IoU >= threshold."""
    ious = np.asarray(ious, dtype=np.float64)
    return float((ious >= threshold).sum()) / float(len(ious)) * 100.0


def summarise(ious, epoch=None, global_step=None):
    """The metric block of eval_test (runner_utils_t7.py:90-101) -> (r1i3, r1i5, r1i7, mIoU, score string)."""
    r1i3, r1i5, r1i7 = (calculate_iou_accuracy(ious, t) for t in (0.3, 0.5, 0.7))
    mi = float(np.mean(ious) * 100.0)
    text = 'Epoch {}, Step {}:\n'.format(epoch, global_step)
    text += 'Rank@1, IoU=0.3: {:.2f}\tRank@1, IoU=0.5: {:.2f}\tRank@1, IoU=0.7: {:.2f}\tmean IoU: {:.2f}\n'.format(r1i3, r1i5, r1i7, mi)
    return r1i3, r1i5, r1i7, mi, text


def best_iou_of_spans(start, end, count, record):
    """The best IoU with the record's ground truth over the first `count` spans of one sample (0 when there is none)."""
    gt = [record['s_time'], record['e_time']]
    return max([calculate_iou([st, et], gt) for st, et in spans_to_times(start, end, count, record['v_len'], record['duration'])], default=0.0)


def summarise_topk(best_ious, k):
    """Rank@K: the share of samples whose best IoU over their K spans reaches the threshold -> ({'k', 'r_k_i3', 'r_k_i5', 'r_k_i7', 'mIoU_k'}, text line)."""
    r3, r5, r7 = (calculate_iou_accuracy(best_ious, t) for t in (0.3, 0.5, 0.7))
    mi = float(np.mean(best_ious) * 100.0)
    text = 'Rank@{k}, IoU=0.3: {:.2f}\tIoU=0.5: {:.2f}\tIoU=0.7: {:.2f}\tbest-of-{k} mean IoU: {:.2f}\n'.format(r3, r5, r7, mi, k=k)
    return {'k': k, 'r_k_i3': r3, 'r_k_i5': r5, 'r_k_i7': r7, 'mIoU_k': mi}, text


def _spans_to_host(s_idx, e_idx, spans):
    """The indices of extract_index and, with `spans`, the (B, K) starts / ends and the counts of extract_topk, in ONE device-to-host copy."""
    if spans is None:
        idx = torch.stack([s_idx, e_idx]).cpu().numpy()
        return idx[0], idx[1], None
    K = spans.start.shape[1]
    out = torch.cat([s_idx[:, None], e_idx[:, None], spans.start, spans.end, spans.count[:, None].long()], dim=1).cpu().numpy()
    return out[:, 0], out[:, 1], (out[:, 2:2 + K], out[:, 2 + K:2 + 2 * K], out[:, 2 + 2 * K])


def _finish(ious, best, topk, epoch, global_step):
    out = summarise(ious, epoch, global_step)
    if topk is None:
        return out
    stats, line = summarise_topk(best, topk.k)
    return out[:4] + (out[4] + line, stats)


def eval_test(model, data_loader, device, mode='test', epoch=None, global_step=None, topk=None):
    """runner_utils_t7.py:71-101.  The batch is moved with non-blocking copies (pinned staging when the loader pins), the
    indices of the whole batch come back in one D2H copy.
    `topk` (a TopK(k, nms_iou, max_span); no reference counterpart): the loop also asks for the k best moments per query (VSLNet.extract_topk) and
    returns a sixth value, the Rank@K dict of summarise_topk, with one more line in the text; the first four values stay those of extract_index."""
    del mode
    ious, best = [], []
    with torch.no_grad():
        for records, vfeats, vfeat_lens, word_ids, char_ids in data_loader:
            vfeats, vfeat_lens = vfeats.to(device, non_blocking=True), vfeat_lens.to(device, non_blocking=True)
            word_ids, char_ids = word_ids.to(device, non_blocking=True), char_ids.to(device, non_blocking=True)
            query_mask = (word_ids != 0).float()
            video_mask = convert_length_to_mask(vfeat_lens)
            _, start_logits, end_logits = model(word_ids, char_ids, vfeats, video_mask, query_mask)
            s_idx, e_idx = model.extract_index(start_logits, end_logits)
            spans = None if topk is None else model.extract_topk(start_logits, end_logits, topk.k, nms_iou=topk.nms_iou, max_span=topk.max_span,
                                                                 v_mask=video_mask, want_prob=False)
            s_host, e_host, sp = _spans_to_host(s_idx, e_idx, spans)
            for n, (r, si, ei) in enumerate(zip(records, s_host, e_host)):
                st, et = index_to_time(int(si), int(ei), r['v_len'], r['duration'])
                ious.append(calculate_iou([st, et], [r['s_time'], r['e_time']]))
                if sp is not None:
                    best.append(best_iou_of_spans(sp[0][n], sp[1][n], sp[2][n], r))
    return _finish(ious, best, topk, epoch, global_step)


def eval_test_shared(model, split, device, mode='test', epoch=None, global_step=None, videos_per_call=64, topk=None):
    """eval_test over a `data.ResidentSplit` with every video encoded ONCE (split.encode -> VSLNet.encode_video) and each batch of records
    localised against that resident encoding (VSLNet.localize with the records' video indices): no (B, T, Dv) feature block is gathered and
    VisualProjection + the video pass of the feature encoder run once per video instead of once per record.  Returns what eval_test returns
    (`topk` as there; the valid lengths are the split's clips per record).
    An encoding belongs to its padded T, so every batch runs at the split's Tmax: the numbers are those of evaluating with every batch padded to
    Tmax -- what `model(...)` gives on `split.feats[:, :Tmax][vid]` -- not to the batch maximum as eval_test pads; the two differ, because the
    conv block's zero padding at the sequence end turns into pad-row values that the attention spreads to every row."""
    del mode, device
    ious, best = [], []
    bs, n = split.batch_size, len(split.records)
    with torch.no_grad():
        enc = split.encode(model, videos_per_call=videos_per_call)
        d_order = torch.arange(n, device=split.device)
        for a in range(0, n, bs):
            idx = np.arange(a, min(n, a + bs))
            idx_dev = d_order[a:a + bs]
            Lq, Lc = int(split.nwords[idx].max()), int(split.nchars[idx].max())
            word_ids = torch.index_select(split.d_words[:, :Lq], 0, idx_dev)
            char_ids = torch.index_select(split.d_chars[:, :Lq, :Lc], 0, idx_dev)
            query_mask = (word_ids != 0).float()
            _, start_logits, end_logits = model.localize(enc, split.vid_of[idx], word_ids, char_ids, query_mask, T=enc.T)
            s_idx, e_idx = model.extract_index(start_logits, end_logits)
            spans = None if topk is None else model.extract_topk(start_logits, end_logits, topk.k, nms_iou=topk.nms_iou, max_span=topk.max_span,
                                                                 lengths=torch.index_select(split.d_lens, 0, idx_dev), want_prob=False)
            s_host, e_host, sp = _spans_to_host(s_idx, e_idx, spans)
            for m, (i, si, ei) in enumerate(zip(idx, s_host, e_host)):
                r = split.records[i]
                st, et = index_to_time(int(si), int(ei), r['v_len'], r['duration'])
                ious.append(calculate_iou([st, et], [r['s_time'], r['e_time']]))
                if sp is not None:
                    best.append(best_iou_of_spans(sp[0][m], sp[1][m], sp[2][m], r))
    return _finish(ious, best, topk, epoch, global_step)


def summarise_windows(ious, best, window, stride, topk):
    """The metric block of eval_windows -> (stats dict, text): Rank@1 at IoU 0.3 / 0.5 / 0.7 and mean IoU of the first merged moment, and with `topk`
    Rank@K over the K merged moments."""
    r3, r5, r7 = (calculate_iou_accuracy(ious, t) for t in (0.3, 0.5, 0.7))
    mi = float(np.mean(ious) * 100.0)
    stats = {'window': int(window), 'window_stride': int(stride), 'win_r1i3': r3, 'win_r1i5': r5, 'win_r1i7': r7, 'win_mIoU': mi}
    text = 'Windows {}/{}: Rank@1, IoU=0.3: {:.2f}\tIoU=0.5: {:.2f}\tIoU=0.7: {:.2f}\tmean IoU: {:.2f}\n'.format(window, stride, r3, r5, r7, mi)
    if topk is not None:
        sk, line = summarise_topk(best, topk.k)
        stats.update({'win_' + key: v for key, v in sk.items() if key != 'k'})
        text += 'Windows {}/{}: '.format(window, stride) + line
    return stats, text


def eval_windows(model, split, device, window, stride, topk=None, windows_per_call=256, pairs_per_call=4096):
    """Evaluation by sliding windows (no reference counterpart): every video of a `data.ResidentSplit` is encoded as overlapping windows of `window`
    clips at `stride` over the clip sequence the split holds (VSLNet.encode_windows, once), each batch of records encodes its queries
    (VSLNet.encode_query) and VSLNet.localize_long returns each record's merged moments in its video's own clips; one device-to-host copy per batch
    brings (start, end, count) back.  Rank@1 / mean IoU are those of the FIRST merged moment, Rank@K (with `topk`, whose nms_iou / max_span also
    act inside and across the windows) of the best of the K; times through index_to_time with the video's full clip count.
    -> (stats dict, text) of summarise_windows."""
    del device
    k = 1 if topk is None else topk.k
    nms_iou, max_span = (0.5, 0) if topk is None else (topk.nms_iou, topk.max_span)
    ious, best = [], []
    bs, n = split.batch_size, len(split.records)
    with torch.no_grad():
        vlen = np.zeros(int(split.feats.shape[0]), dtype=np.int64)
        vlen[split.vid_of] = split.lens
        wenc = model.encode_windows([split.feats[v, :int(vlen[v])] for v in range(len(vlen))], window, stride, windows_per_call=windows_per_call)
        d_order = torch.arange(n, device=split.device)
        for a in range(0, n, bs):
            idx = np.arange(a, min(n, a + bs))
            idx_dev = d_order[a:a + bs]
            Lq, Lc = int(split.nwords[idx].max()), int(split.nchars[idx].max())
            word_ids = torch.index_select(split.d_words[:, :Lq], 0, idx_dev)
            char_ids = torch.index_select(split.d_chars[:, :Lq, :Lc], 0, idx_dev)
            qenc = model.encode_query(word_ids, char_ids, (word_ids != 0).float())
            m = model.localize_long(wenc, qenc, k, nms_iou=nms_iou, max_span=max_span, pairs=np.stack([split.vid_of[idx], np.arange(len(idx))], axis=1),
                                    pairs_per_call=pairs_per_call)
            out = torch.cat([m.start, m.end, m.count[:, None].long()], dim=1).cpu().numpy()
            for q, i in enumerate(idx):
                r = split.records[i]
                b = best_iou_of_spans(out[q, :k], out[q, k:2 * k], out[q, 2 * k], r)
                ious.append(best_iou_of_spans(out[q, :1], out[q, k:k + 1], min(int(out[q, 2 * k]), 1), r))
                best.append(b)
    return summarise_windows(ious, best, window, stride, topk)


def corpus_hits(tag, start, end, count, record, video):
    """One query's corpus result against its record: the best IoU over the returned moments that lie in the ground-truth video `video` (0 when none
    does) and whether any does.  A moment in another video is a miss whatever its span."""
    gt = [record['s_time'], record['e_time']]
    inside = [r for r in range(int(count)) if int(tag[r]) == int(video)]
    best = max([calculate_iou(list(index_to_time(int(start[r]), int(end[r]), record['v_len'], record['duration'])), gt) for r in inside], default=0.0)
    return best, bool(inside)


def summarise_corpus(best_ious, found, k):
    """Corpus Rank@K: the share of queries with a returned moment IN THE GROUND-TRUTH VIDEO at IoU >= 0.5 / 0.7, and video Recall@K: the share with any
    returned moment in that video -> ({'k', 'corpus_r_k_i5', 'corpus_r_k_i7', 'video_recall_k'}, text line)."""
    r5, r7 = (calculate_iou_accuracy(best_ious, t) for t in (0.5, 0.7))
    rec = float(np.mean(np.asarray(found, dtype=np.float64)) * 100.0)
    text = 'Corpus Rank@{k}, IoU=0.5: {:.2f}\tIoU=0.7: {:.2f}\tvideo Recall@{k}: {:.2f}\n'.format(r5, r7, rec, k=k)
    return {'k': k, 'corpus_r_k_i5': r5, 'corpus_r_k_i7': r7, 'video_recall_k': rec}, text


def eval_corpus(model, split, device, topk, videos_per_call=64, pairs_per_call=4096, prefilter=0, relevance='max'):
    """Moment retrieval over the whole split (no reference counterpart): every record's query is run against EVERY video of a `data.ResidentSplit`,
    not only its own.  The videos are encoded once at the split's Tmax (split.encode, as eval_test_shared does), the queries batch by batch
    (VSLNet.encode_query), and VSLNet.retrieve returns each query's topk.k best moments over all videos, ranked on the device; one device-to-host
    copy per batch brings (video, start, end, count) back.  -> (stats dict, text line) of summarise_corpus.  `topk`: a TopK(k, nms_iou, max_span).
    `prefilter` = M >= 1 (with `relevance`): VSLNet.retrieve's coarse-to-fine search, localising in the M best videos per query only.  The stats
    then also hold 'prefilter_m' and 'prefilter_recall_m' -- prefilter video recall@M: the share of queries whose ground-truth video is among the M
    selected (the first stage's VideoRanks; the set comes back in the same copy as the moments) -- and the text starts with that line."""
    del device
    if topk is None:
        raise ValueError('eval_corpus needs topk = TopK(k >= 1, nms_iou, max_span): the moments returned per query')
    prefilter = int(prefilter or 0)
    best, found, kept = [], [], []
    bs, n = split.batch_size, len(split.records)
    with torch.no_grad():
        venc = split.encode(model, videos_per_call=videos_per_call)
        d_order = torch.arange(n, device=split.device)
        for a in range(0, n, bs):
            idx = np.arange(a, min(n, a + bs))
            idx_dev = d_order[a:a + bs]
            Lq, Lc = int(split.nwords[idx].max()), int(split.nchars[idx].max())
            word_ids = torch.index_select(split.d_words[:, :Lq], 0, idx_dev)
            char_ids = torch.index_select(split.d_chars[:, :Lq, :Lc], 0, idx_dev)
            qenc = model.encode_query(word_ids, char_ids, (word_ids != 0).float())
            per_call = max(pairs_per_call, len(idx))
            if prefilter:
                m, ranks = model.retrieve(venc, qenc, topk.k, nms_iou=topk.nms_iou, max_span=topk.max_span, pairs_per_call=per_call, prefilter=prefilter,
                                          relevance=relevance, return_ranks=True)
                out = torch.cat([m.tag.long(), m.start, m.end, m.count[:, None].long(), ranks.video.long()], dim=1).cpu().numpy()
            else:
                m = model.retrieve(venc, qenc, topk.k, nms_iou=topk.nms_iou, max_span=topk.max_span, pairs_per_call=per_call)
                out = torch.cat([m.tag.long(), m.start, m.end, m.count[:, None].long()], dim=1).cpu().numpy()
            K = topk.k
            for q, i in enumerate(idx):
                b, f = corpus_hits(out[q, :K], out[q, K:2 * K], out[q, 2 * K:3 * K], out[q, 3 * K], split.records[i], split.vid_of[i])
                best.append(b)
                found.append(f)
                if prefilter:
                    kept.append(int(split.vid_of[i]) in out[q, 3 * K + 1:].tolist())
    stats, text = summarise_corpus(best, found, topk.k)
    if prefilter:
        rec = float(np.mean(np.asarray(kept, dtype=np.float64)) * 100.0)
        stats = dict(stats, prefilter_m=prefilter, prefilter_recall_m=rec)
        text = 'Prefilter ({}) video recall@{}: {:.2f}\n'.format(relevance, prefilter, rec) + text
    return stats, text
