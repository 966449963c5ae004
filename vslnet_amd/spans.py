"""Top-K moments per query: the written specifications of `vsl_extract_topk`, `vsl_merge_topk` and `vsl_merge_windows` (include/vslnet_hip.h) as
brute-force numpy, the table of sliding windows over a video, and the conversion of spans to seconds.  `topk_spans_reference`, `merge_topk_reference`
and `merge_windows_reference` are what the tests compare the kernels with; the library never calls them."""
from collections import namedtuple

import numpy as np

from .data import index_to_time

# the evaluation loops' switch (runner.eval_test / eval_test_shared, main.py --topk / --nms_iou / --max_span)
TopK = namedtuple('TopK', 'k nms_iou max_span')
TopK.__new__.__defaults__ = (1.0, 0)


def suppressed(s, e, cs, ce, nms_iou):
    """Is the candidate span (s, e) suppressed by the chosen (cs, ce)?  Spans are clip intervals [s, e + 1); the compare is the kernel's: two
    integers exact in float32 and ONE float32 multiply."""
    inter = max(0, min(e, ce) - max(s, cs) + 1)
    uni = (e - s + 1) + (ce - cs + 1) - inter
    return inter > 0 and bool(np.float32(inter) > np.float32(nms_iou) * np.float32(uni))


def topk_spans_reference(sl, el, k, nms_iou=1.0, max_span=0, lengths=None):
    """(B, T) float32 logits -> start, end (B, k) int64, score (B, k) float32, prob (B, k) float64, count (B,) int32.
    Per sample, L = lengths[b] clamped into [1, T] (T without lengths); candidates (s, e), 0 <= s <= e < L, e - s + 1 <= max_span when max_span > 0;
    score = sl[s] + el[e] as one float32 addition; k greedy rounds, each taking the first maximum in row-major order of the candidates that are
    neither chosen nor suppressed by an earlier choice (`suppressed`).  prob = exp(score - lse(sl) - lse(el)) in float64 over the sample's T
    logits.  Slots from count on hold -1, -1, -inf, 0."""
    sl, el = np.ascontiguousarray(sl, dtype=np.float32), np.ascontiguousarray(el, dtype=np.float32)
    B, T = sl.shape
    start, end = np.full((B, k), -1, dtype=np.int64), np.full((B, k), -1, dtype=np.int64)
    score, prob = np.full((B, k), -np.inf, dtype=np.float32), np.zeros((B, k), dtype=np.float64)
    count = np.zeros(B, dtype=np.int32)
    si, ei = np.arange(T)[:, None], np.arange(T)[None, :]
    for b in range(B):
        L = T if lengths is None else min(max(int(lengths[b]), 1), T)
        live = (si <= ei) & (ei < L)
        if max_span > 0:
            live &= ei - si + 1 <= max_span
        sc = sl[b][:, None] + el[b][None, :]                     # float32 + float32 -> float32: one rounding
        lse = [float(np.log(np.exp(x.astype(np.float64) - float(x.max())).sum()) + float(x.max())) for x in (sl[b], el[b])]
        ln = (ei - si + 1).astype(np.float32)
        for r in range(k):
            if not live.any():
                break
            pick = int(np.argmax(np.where(live, sc, -np.inf)))   # argmax: the first maximum in row-major order (start ascending, then end ascending)
            if not live.reshape(-1)[pick]:                       # (every live score is -inf: the first live candidate)
                pick = int(np.flatnonzero(live)[0])
            cs, ce = divmod(pick, T)
            start[b, r], end[b, r], score[b, r] = cs, ce, sc[cs, ce]
            prob[b, r] = np.exp(float(sc[cs, ce]) - lse[0] - lse[1])
            count[b] = r + 1
            live[cs, ce] = False
            inter = np.maximum(0, np.minimum(ei, ce) - np.maximum(si, cs) + 1)
            uni = ln + np.float32(ce - cs + 1) - inter.astype(np.float32)
            live &= ~((inter > 0) & (inter.astype(np.float32) > np.float32(nms_iou) * uni))
    return start, end, score, prob, count


def merge_topk_reference(start, end, score, key, count, group_index, G, k_out, tag=None):
    """B lists of K slots -> per group g: tag, list (G, k_out) int32, start, end (G, k_out) int64, score, key (G, k_out) float32, count (G,) int32.
    Candidates of group g: slot k < min(count[b], K) of every list b with group_index[b] == g (a group_index outside [0, G): no group).  A candidate's
    tag is tag[b], tag[b][k] for a (B, K) tag, b without one.  They are sorted by key descending, then tag, list and slot ascending -- a strict total
    order -- and the first k_out are written.  Slots from count[g] on hold -1, -1, -1, -1, -inf, 0."""
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    score, key = np.asarray(score, dtype=np.float32), np.asarray(key, dtype=np.float32)
    B, K = start.shape
    tag = None if tag is None else np.asarray(tag)
    out_tag, out_list = np.full((G, k_out), -1, dtype=np.int32), np.full((G, k_out), -1, dtype=np.int32)
    out_start, out_end = np.full((G, k_out), -1, dtype=np.int64), np.full((G, k_out), -1, dtype=np.int64)
    out_score, out_key = np.full((G, k_out), -np.inf, dtype=np.float32), np.zeros((G, k_out), dtype=np.float32)
    out_count = np.zeros(G, dtype=np.int32)
    cands = [[] for _ in range(G)]
    for b in range(B):
        g = int(group_index[b])
        if not 0 <= g < G:
            continue
        for k in range(min(int(count[b]), K)):
            t = b if tag is None else int(tag[b, k]) if tag.ndim == 2 else int(tag[b])
            cands[g].append((-float(key[b, k]), t, b, k))
    for g in range(G):
        for r, (_, t, b, k) in enumerate(sorted(cands[g])[:k_out]):
            out_tag[g, r], out_list[g, r], out_start[g, r], out_end[g, r] = t, b, start[b, k], end[b, k]
            out_score[g, r], out_key[g, r] = score[b, k], key[b, k]
            out_count[g] = r + 1
    return out_tag, out_list, out_start, out_end, out_score, out_key, out_count


def pair_relevance_reference(h_score, v_mask_or_lengths, mode='max', fp32_order=False):
    """(B, T) highlight scores -> (B,) float32: one relevance per pair over its VALID clips (vsl_highlight_pairs).  Validity: a (B, T) mask (non-zero =
    valid) or (B,) lengths (the first lengths[b] clips).  mode 'max': the maximum, exact; 'mean': sum / count in float64, rounded once to float32 (the
    kernel sums in fp32: compare with a tolerance).  A pair without a valid clip gets -inf.
    fp32_order=True: the mean as the device forms it, addition for addition (rank_reduce.hpp pair_row_reduce): 64 fp32 partials, partial l over the
    valid clips l, l + 64, ... ascending, joined by a six-step xor butterfly (32, 16, .., 1), then ONE fp32 division -- the device's bits."""
    if mode not in ('max', 'mean'):
        raise ValueError("relevance must be 'max' or 'mean', got %r" % (mode,))
    h = np.asarray(h_score, dtype=np.float32)
    B, T = h.shape
    v = np.asarray(v_mask_or_lengths)
    valid = (v != 0) if v.ndim == 2 else (np.arange(T)[None, :] < v.reshape(B, 1))
    out = np.full(B, -np.inf, dtype=np.float32)
    for b in range(B):
        x = h[b][valid[b]]
        if x.size:
            if mode == 'max':
                out[b] = x.max()
            elif not fp32_order:
                out[b] = np.float32(x.astype(np.float64).sum() / x.size)
            else:
                part = np.zeros(64, dtype=np.float32)
                for t in np.flatnonzero(valid[b]):
                    part[t % 64] = part[t % 64] + h[b, t]            # (float32 + float32 -> float32: one rounding)
                for step in (32, 16, 8, 4, 2, 1):
                    part = part + part[np.arange(64) ^ step]
                out[b] = part[0] / np.float32(x.size)
    return out


GroupLoss = namedtuple('GroupLoss', 'losses hits relevance d_h d_sl d_el')


def group_loss_reference(h_score, start_logits, end_logits, v_mask, start_labels, end_labels, h_labels, group_start, positive, w_loc=1.0,
                         w_highlight=5.0, w_rank=1.0, temperature=0.1, relevance='max', inv_pos=None, inv_groups=None, mask_sum=0.0):
    """The written specification of vsl_group_loss (include/vslnet_hip.h) in float64 -> GroupLoss(losses (5,) float64: loc, highlight, rank, total,
    mask sum used; hits int; relevance (B,) float32; d_h, d_sl, d_el (B, T) float64).  B pair rows in G contiguous groups, group g = rows
    group_start[g] .. group_start[g + 1] - 1 with its true pair at row positive[g].  Everything is float64 on the float32 inputs EXCEPT the relevance,
    which is pair_relevance_reference(fp32_order=True): the device's own float32 value, so that z = r / temperature carries no reduction error of
    this function's.  `start_labels` / `end_labels` (read at positive rows only) and `h_labels` may be None with a zero weight.  inv_pos and
    inv_groups default to 1 / G; mask_sum <= 0: the sum of v_mask."""
    h = np.asarray(h_score, dtype=np.float32)
    B, T = h.shape
    m = np.asarray(v_mask, dtype=np.float32).astype(np.float64)
    gs, pos = np.asarray(group_start, dtype=np.int64), np.asarray(positive, dtype=np.int64)
    G = pos.size
    if gs.size != G + 1 or gs[0] != 0 or gs[-1] != B or (np.diff(gs) < 1).any() or ((pos < gs[:-1]) | (pos >= gs[1:])).any():
        raise ValueError('group_loss_reference: group_start / positive do not cut %d rows into %d non-empty groups with their positive rows' % (B, G))
    if (start_labels is None or end_labels is None) and w_loc != 0 or h_labels is None and w_highlight != 0:
        raise ValueError('group_loss_reference: labels may be None only with a zero weight')
    inv_pos = 1.0 / G if inv_pos is None else float(inv_pos)
    inv_groups = 1.0 / G if inv_groups is None else float(inv_groups)
    inv_t = float(np.float32(1.0 / temperature))                  # (what the caller hands the device)
    d_h, d_sl, d_el = np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T))
    # span: CE(start) + CE(end) over the positive rows
    ce = 0.0
    if start_labels is not None and end_labels is not None:
        for x, lab, d in ((start_logits, start_labels, d_sl), (end_logits, end_labels, d_el)):
            x = np.asarray(x, dtype=np.float32).astype(np.float64)
            for b in pos:
                lse = np.log(np.exp(x[b] - x[b].max()).sum()) + x[b].max()
                ce += lse - x[b, int(lab[b])]
                d[b] = w_loc * inv_pos * np.exp(x[b] - lse)
                d[b, int(lab[b])] -= w_loc * inv_pos
    loc = ce * inv_pos
    # highlight: the weighted BCE over all rows (BCELoss clamps its logs at -100)
    den = float(mask_sum) if mask_sum > 0 else float(m.sum())
    hl = 0.0
    if h_labels is not None:
        y = np.asarray(h_labels).astype(np.float64)
        p = h.astype(np.float64)
        q = 1.0 - p
        with np.errstate(divide='ignore'):
            lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log(q), -100.0)
        w = np.where(y == 0, 1.0, 2.0 * y)
        hl = float((-(y * lp + (1.0 - y) * lq) * w * m).sum() / (den + 1e-12))
        d_h += w_highlight * w * m / (den + 1e-12) * (p - y) / np.maximum(p * q, 1e-12)
    # rank: softmax over every group's relevances
    rel = pair_relevance_reference(h, v_mask, relevance, fp32_order=True)
    valid = np.asarray(v_mask) != 0
    z = rel.astype(np.float64) * inv_t
    rank, hits = 0.0, 0
    for g in range(G):
        rows = [b for b in range(gs[g], gs[g + 1]) if np.isfinite(z[b])]
        pb = int(pos[g])
        if not np.isfinite(z[pb]):
            continue                                              # skipped: the positive row has no valid clip
        zz = z[rows]
        lse = np.log(np.exp(zz - zz.max()).sum()) + zz.max()
        rank += lse - z[pb]
        hits += int(min(rows, key=lambda b: (-z[b], b)) == pb)
        for b in rows:
            dr = w_rank * inv_groups * inv_t * (np.exp(z[b] - lse) - (b == pb))
            if relevance == 'max':
                d_h[b, int(np.flatnonzero(valid[b] & (h[b] == rel[b]))[0])] += dr
            else:
                d_h[b, valid[b]] += dr / valid[b].sum()
    rank *= inv_groups
    losses = np.array([loc, hl, rank, w_loc * loc + w_highlight * hl + w_rank * rank, den])
    return GroupLoss(losses, hits, rel, d_h, d_sl, d_el)


def select_topm_reference(key, M):
    """(G, N) keys -> index (G, M) int32, key (G, M) float32, count (G,) int32: per row the first min(M, N) indices in the order key descending, ties by
    the smaller index, ranked (vsl_select_topm).  -0.0 counts as +0.0: keys are compared -- and returned -- as key + 0.0.  Slots from count on: -1, 0."""
    key = np.asarray(key, dtype=np.float32) + np.float32(0.0)
    G, N = key.shape
    n = min(int(M), N)
    out_index, out_key = np.full((G, M), -1, dtype=np.int32), np.zeros((G, M), dtype=np.float32)
    index = np.arange(N)
    for g in range(G):
        order = np.lexsort((index, -key[g]))[:n]
        out_index[g, :n], out_key[g, :n] = order, key[g][order]
    return out_index, out_key, np.full(G, n, dtype=np.int32)


def window_table(L, window, stride):
    """The sliding windows over a video of L clips -> (start, length) int64 arrays: window w starts at clip w * stride; there is one window when
    L <= window, else ceil((L - window) / stride) + 1; the last one may be short: length = min(window, L - w * stride).  Every clip is covered when
    stride <= window."""
    L, window, stride = int(L), int(window), int(stride)
    if L < 1 or window < 1 or stride < 1:
        raise ValueError('window_table: L=%d, window=%d, stride=%d must all be at least 1' % (L, window, stride))
    if stride > window:
        raise ValueError('window_table: stride=%d > window=%d would skip clips' % (stride, window))
    W = 1 if L <= window else -(-(L - window) // stride) + 1
    start = np.arange(W, dtype=np.int64) * stride
    return start, np.minimum(window, L - start)


def merge_windows_reference(start, end, score, key, count, group_index, G, k_out, nms_iou, offset=None):
    """B lists of K slots at window-local indices -> per group g: list (G, k_out) int32, start, end (G, k_out) int64 in GLOBAL clips, score, key
    (G, k_out) float32, count (G,) int32.  Candidates of group g: slot k < min(count[b], K) of every list b with group_index[b] == g (outside [0, G): no
    group), at the global span (start + offset[b], end + offset[b]) (offset None: 0).  They are sorted by key descending, then global start, global
    end, list and slot ascending -- a strict total order; k_out rounds each take the first candidate in that order that no earlier choice of the group
    suppresses: a chosen span suppresses a candidate iff the two global spans are identical (at every nms_iou) or `suppressed` holds on them.  Slots
    from count[g] on hold -1, -1, -1, -inf, 0."""
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    score, key = np.asarray(score, dtype=np.float32), np.asarray(key, dtype=np.float32)
    B, K = start.shape
    offset = np.zeros(B, dtype=np.int64) if offset is None else np.asarray(offset, dtype=np.int64)
    out_list = np.full((G, k_out), -1, dtype=np.int32)
    out_start, out_end = np.full((G, k_out), -1, dtype=np.int64), np.full((G, k_out), -1, dtype=np.int64)
    out_score, out_key = np.full((G, k_out), -np.inf, dtype=np.float32), np.zeros((G, k_out), dtype=np.float32)
    out_count = np.zeros(G, dtype=np.int32)
    cands = [[] for _ in range(G)]
    for b in range(B):
        g = int(group_index[b])
        if not 0 <= g < G:
            continue
        for k in range(min(int(count[b]), K)):
            cands[g].append((-float(key[b, k]), int(start[b, k] + offset[b]), int(end[b, k] + offset[b]), b, k))
    for g in range(G):
        chosen = []
        for _, s, e, b, k in sorted(cands[g]):
            if len(chosen) == k_out:
                break
            if any((s, e) == (cs, ce) or suppressed(s, e, cs, ce, nms_iou) for cs, ce in chosen):
                continue
            r = len(chosen)
            chosen.append((s, e))
            out_list[g, r], out_start[g, r], out_end[g, r], out_score[g, r], out_key[g, r] = b, s, e, score[b, k], key[b, k]
            out_count[g] = r + 1
    return out_list, out_start, out_end, out_score, out_key, out_count


def spans_to_times(start, end, count, v_len, duration):
    """The first `count` spans of one sample (clip indices) -> [(start_time, end_time)] in seconds, through data.index_to_time."""
    return [index_to_time(int(s), int(e), v_len, duration) for s, e in zip(start[:int(count)], end[:int(count)])]
