"""Sliding windows over a video of any length, the GPU half: vsl_encode_windows (each clip projected once, each window encoded) against vsl_encode_video on
the materialised zero-padded windows, bit for bit; vsl_merge_windows (shift, rank and suppress across windows) against its written specification
(vslnet_amd.spans.merge_windows_reference), bit for bit; VSLNet.encode_windows / localize_long against the composition of the calls they replace; the
handles' staleness rules; every refusal by its message.  The CPU half (specification, window table, exports) is tests/test_windows_spec.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from vslnet_amd.spans import merge_windows_reference, topk_spans_reference, window_table

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _model(Dv=64, heads=8, max_pos_len=40, seed=811):
    from tests.test_shared_video import _module
    cfg = O.make_cfg(video_feature_dim=Dv, max_pos_len=max_pos_len, word_size=102, num_heads=heads)
    P = O.random_params(cfg, seed=seed)
    bias = [v for k, v in P.items() if k.startswith('video_affine') and 'bias' in k]
    assert bias and float(bias[0].abs().min()) > 0                # a pad row of a window is the bias: it must not be zero here
    return cfg, P, _module(cfg, P).to('cuda').eval()


def _videos(Dv, lengths, seed, bf16=False):
    rng = np.random.default_rng(seed)
    vids = [torch.from_numpy(rng.standard_normal((L, Dv)).astype(np.float32)).cuda() for L in lengths]
    return [v.to(torch.bfloat16) for v in vids] if bf16 else vids


def _materialise(videos, window, stride):
    """the (N, window, Dv) block of zero-padded windows the library never builds, its mask, and the tables"""
    blocks, masks, video_of, offset, wlen = [], [], [], [], []
    for i, v in enumerate(videos):
        start, length = window_table(v.shape[0], window, stride)
        for s, n in zip(start.tolist(), length.tolist()):
            x = torch.zeros(window, v.shape[1], dtype=v.dtype, device=v.device)
            x[:n] = v[s:s + n]
            blocks.append(x)
            masks.append((torch.arange(window, device=v.device) < n).float())
            video_of.append(i), offset.append(s), wlen.append(n)
    return torch.stack(blocks), torch.stack(masks), np.array(video_of), np.array(offset), np.array(wlen)


def _queries(cfg, Q, seed, Lq=7, Lc=6):
    qb = O.synthetic_batch(cfg, Q, 8, Lq, Lc, seed=seed, ragged=True)
    return qb['word_ids'].cuda(), qb['char_ids'].cuda(), qb['q_mask'].cuda()


# ------------------------------------------------------------------------------------------------ 1. the encoding, bit for bit
#               Dv  heads lengths    window stride bf16
ENCODE_CASES = [(20, 8, (75,), 32, 16, False),                   # four windows, the last with 27 clips ; a feature width below one K chunk
                (64, 8, (75,), 32, 16, False),
                (128, 8, (75,), 32, 16, False),                  # 75 rows: the ragged projection kernel ; 4 x 32 materialised rows: the whole-tile one
                (64, 8, (24,), 24, 24, False),                   # a single full window under one tile
                (64, 8, (10,), 32, 16, False),                   # a video shorter than a window
                (64, 8, (60,), 37, 5, False),                    # off the 32-row tile, six windows
                (64, 8, (75, 40), 32, 16, False),                # two videos in one call
                (64, 8, (75, 40), 32, 16, True),                 # bf16 features
                (64, 4, (75,), 32, 16, False)]                   # 4 heads


@pytest.mark.parametrize('case', ENCODE_CASES, ids=lambda c: 'Dv%d-h%d-L%s-w%d-s%d%s' % (c[0], c[1], '_'.join(map(str, c[2])), c[3], c[4], '-bf16' if c[5] else ''))
def test_encode_windows_equals_encode_video_on_the_materialised_windows(case):
    from vslnet_amd.engine import VideoEncoding, WindowEncoding
    Dv, heads, lengths, window, stride, bf16 = case
    cfg, P, m = _model(Dv, heads)
    videos = _videos(Dv, lengths, seed=sum(lengths) + window, bf16=bf16)
    X, mask, video_of, offset, wlen = _materialise(videos, window, stride)
    with torch.no_grad():
        ref = m.encode_video(X, mask)
        got = m.encode_windows(videos if len(videos) > 1 else videos[0], window, stride)
        three = m.encode_windows(videos, window, stride, windows_per_call=3)
    assert isinstance(got, WindowEncoding) and isinstance(got, VideoEncoding) and (got.N, got.T) == (len(wlen), window)
    assert torch.equal(got.v_mask, mask)
    diff = float((got.encoding - ref.encoding).abs().max())
    print('encode_windows vs encode_video: max |diff| %g over %s' % (diff, tuple(ref.encoding.shape)))
    assert torch.equal(got.encoding, ref.encoding), diff
    assert got.video_of_window.cpu().tolist() == video_of.tolist() and got.offset_of_window.cpu().tolist() == offset.tolist()
    assert got.window_len.cpu().tolist() == wlen.tolist() and got.lengths.tolist() == list(lengths)
    assert got.first_window.tolist() == [0] + np.cumsum(np.bincount(video_of, minlength=len(lengths))).tolist()
    assert got.owner is m and got.epoch == m._param_epoch and (got.window, got.stride) == (window, stride)
    assert torch.equal(three.v_mask, mask)
    if window % 32 == 0 or window <= 32:                         # a window's batch position changes with the chunking: exact where the encoder ignores it
        assert torch.equal(three.encoding, got.encoding)
    else:                                                        # off the tile: the golden gate of tests/test_shared_video.py's off-tile cases
        scale = max(1.0, float(got.encoding.abs().max()))
        assert float((three.encoding - got.encoding).abs().max()) < 1e-4 * scale


def test_the_encode_cases_cover_what_they_must():
    assert {(20, 8, (75,), 32, 16), (64, 8, (75,), 32, 16), (64, 8, (24,), 24, 24), (64, 8, (10,), 32, 16), (64, 8, (60,), 37, 5),
            (64, 8, (75, 40), 32, 16)} <= {c[:5] for c in ENCODE_CASES if not c[5]}
    assert any(c[5] for c in ENCODE_CASES) and {c[1] for c in ENCODE_CASES} == {4, 8}
    assert window_table(75, 32, 16)[1].tolist() == [32, 32, 32, 27] and len(window_table(60, 37, 5)[0]) == 6


def test_a_bad_window_table_reads_nothing_outside_the_features():
    """a source row outside [0, rows) is a pad row, whatever the table says"""
    cfg, P, m = _model()
    eng, flat = m._engine_for(torch.device('cuda')), m._flat
    feats = _videos(64, (40,), seed=5)[0]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device='cuda')      # noqa: E731
    with torch.no_grad():
        bad = eng.encode_windows(flat, feats, i32([24, -8, 2 ** 31 - 40]), i32([32, 32, 32]), 32)
        X = torch.zeros(3, 32, 64, device='cuda')
        X[0, :16], X[1, 8:] = feats[24:40], feats[0:24]            # rows 40.. of window 0, rows -8..-1 of window 1 and all of window 2 are padding
        ref = eng.encode_video(flat, X, torch.ones(3, 32, device='cuda'))
    assert torch.equal(bad.v_mask, torch.ones(3, 32, device='cuda')) and torch.equal(bad.encoding, ref.encoding)


# ------------------------------------------------------------------------------------------------ 2. the merge kernel against the specification
@functools.lru_cache(maxsize=None)
def _engine():
    from vslnet_amd.engine import Engine
    return Engine(O.make_cfg(video_feature_dim=64, max_pos_len=32, word_size=52))


def _window_lists(rng, B, K, G, how):
    """B lists of K slots as extract_topk leaves them at window-local indices, keys drawn from 4 values so that ties are dense, offsets on a grid of 8
    clips with starts from a small range so that identical GLOBAL spans occur in several lists"""
    count = rng.integers(0, K + 1, B).astype(np.int32)           # counts include 0
    if B == 1:
        count[:] = K
    start = rng.integers(0, 24, (B, K)).astype(np.int64)
    end = start + rng.integers(0, 6, (B, K))
    score = (3.0 * rng.standard_normal((B, K))).astype(np.float32)
    key = (rng.integers(0, 4, (B, K)) / 4.0).astype(np.float32)
    fill = np.arange(K)[None, :] >= count[:, None]
    start[fill], end[fill], score[fill], key[fill] = -1, -1, -np.inf, 0.0
    offset = (8 * rng.integers(0, 4, B)).astype(np.int32)
    if how == 'all':
        group = np.zeros(B, dtype=np.int32)
    elif how == 'random':
        group = rng.integers(0, G, B).astype(np.int32)
    else:                                                        # group 1 has no list ; -1, G and the extreme ints are no group
        group = rng.choice(np.array([0, 2, -1, G, 2 ** 31 - 1, -2 ** 31]), B).astype(np.int32)
    return (start, end, score, key, count), group, offset


#              B    K   G  K_out group     offset
MERGE_CASES = [(1, 1, 1, 1, 'all', True),                        # B = 1
               (1, 5, 1, 7, 'all', False),
               (600, 5, 3, 7, 'random', True),                   # more lists than threads, three groups
               (600, 1, 3, 32, 'random', True),
               (40, 32, 2, 32, 'random', True),                  # both limits
               (64, 5, 4, 7, 'holes', True),                     # a group with no list, lists in no group
               (64, 5, 4, 1, 'holes', False),                    # offset NULL
               (300, 32, 1, 32, 'all', True)]


def _device_merge(lists, group, offset, G, k_out, nms_iou):
    from vslnet_amd.engine import TopkSpans
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    m = _engine().merge_windows(TopkSpans(*(dev(x) for x in lists)), dev(group), G, k_out, offset=None if offset is None else dev(offset), nms_iou=nms_iou)
    assert (m.list.dtype, m.start.dtype, m.end.dtype, m.score.dtype, m.prob.dtype, m.count.dtype) == \
        (torch.int32, torch.int64, torch.int64, torch.float32, torch.float32, torch.int32)
    return tuple(x.cpu().numpy() for x in m)


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


@pytest.mark.parametrize('nms_iou', [0.0, 0.5, 1.0])
@pytest.mark.parametrize('case', range(len(MERGE_CASES)))
def test_merge_windows_equals_the_specification_bit_for_bit(case, nms_iou):
    B, K, G, k_out, how, with_offset = MERGE_CASES[case]
    lists, group, offset = _window_lists(np.random.default_rng(7000 + case), B, K, G, how)
    offset = offset if with_offset else None
    ref = merge_windows_reference(*lists, group, G, k_out, nms_iou, offset)
    got = _device_merge(lists, group, offset, G, k_out, nms_iou)
    for name, a, r in zip(('list', 'start', 'end', 'score', 'key', 'count'), got, ref):
        assert a.shape == r.shape and np.array_equal(_bits(a), _bits(r)), (MERGE_CASES[case], nms_iou, name, a, r)
    again = _device_merge(lists, group, offset, G, k_out, nms_iou)               # two runs: equal bits
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    if how == 'holes':
        assert ref[5][1] == 0 and (ref[5] > 0).any()
    if B == 600 and K == 5:
        # the data does what the case is for: identical global spans inside a group, and suppression beyond them
        s, e, _, _, count = lists
        live = np.arange(K)[None, :] < count[:, None]
        spans = {(int(g), int(a + o), int(b + o)) for g, a, b, o, ok in zip(np.repeat(group, K), s.reshape(-1), e.reshape(-1), np.repeat(offset, K), live.reshape(-1)) if ok}
        assert len(spans) < int(live.sum())
        assert (lists[4] == 0).any()


def test_the_merge_cases_cover_what_they_must():
    assert {c[1] for c in MERGE_CASES} >= {1, 5, 32} and {c[3] for c in MERGE_CASES} >= {1, 7, 32}
    assert any(c[0] == 1 for c in MERGE_CASES) and any(c[0] == 600 and c[2] == 3 for c in MERGE_CASES)
    assert any(not c[5] for c in MERGE_CASES) and any(c[4] == 'holes' for c in MERGE_CASES)


# ------------------------------------------------------------------------------------------------ 3. end to end
def _host_long(m, videos, window, stride, qenc, k, nms_iou, pairs):
    """the composition localize_long replaces: encode_video on the materialised windows, localize_pairs of every (window, query) of every pair,
    extract_topk per list with the window's length (checked against its own specification), the specification of the cross-window merge on its lists"""
    X, mask, video_of, offset, wlen = _materialise(videos, window, stride)
    venc = m.encode_video(X, mask)
    widx, qidx, group = [], [], []
    for p, (v, q) in enumerate(pairs):
        for w in np.flatnonzero(video_of == v):
            widx.append(int(w)), qidx.append(int(q)), group.append(p)
    _, sl, el = m.localize_pairs(venc, qenc, widx, qidx)
    spans = m.extract_topk(sl, el, k, nms_iou=nms_iou, lengths=wlen[widx])
    s, e, sc, pr, c = (x.cpu().numpy() for x in spans)
    rs, re_, rsc, rpr, rc = topk_spans_reference(sl.cpu().numpy(), el.cpu().numpy(), k, nms_iou, 0, wlen[widx])
    assert np.array_equal(s, rs) and np.array_equal(e, re_) and np.array_equal(sc, rsc) and np.array_equal(c, rc)
    assert float((np.abs(pr - rpr) / (1e-4 * rpr + 1e-7)).max()) <= 1.0
    return merge_windows_reference(s, e, sc, pr, c, np.array(group), len(pairs), k, nms_iou, offset[widx]), np.array(widx)


def test_localize_long_equals_the_composition_it_replaces():
    cfg, P, m = _model()
    videos, k = _videos(64, (75, 40), seed=31), 5
    with torch.no_grad():
        qenc = m.encode_query(*_queries(cfg, 3, seed=32))
        wenc = m.encode_windows(videos, 32, 16)
        got = m.localize_long(wenc, qenc, k, nms_iou=0.5)
        allpairs = [(v, q) for v in range(2) for q in range(3)]
        (lst, s, e, sc, pr, c), widx = _host_long(m, videos, 32, 16, qenc, k, 0.5, allpairs)
        some = [(1, 2), (0, 0), (1, 0), (0, 0)]
        by_pairs = m.localize_long(wenc, qenc, k, nms_iou=0.5, pairs=some)
        chunked = m.localize_long(wenc, qenc, k, nms_iou=0.5, pairs_per_call=6)        # 4 * 3 + 2 * 3 = 18 lists: three chunks
        ref_some = _host_long(m, videos, 32, 16, qenc, k, 0.5, some)[0]
    assert got.start.shape == (6, k) and got.window.dtype == torch.int32 and bool((got.count > 0).all())
    assert torch.equal(got.prob.cpu(), torch.from_numpy(pr))
    assert torch.equal(got.start.cpu(), torch.from_numpy(s)) and torch.equal(got.end.cpu(), torch.from_numpy(e)) and torch.equal(got.count.cpu(), torch.from_numpy(c))
    assert torch.equal(got.score.cpu(), torch.from_numpy(sc))
    assert torch.equal(got.window.cpu(), torch.from_numpy(np.where(lst >= 0, widx[np.maximum(lst, 0)], -1).astype(np.int32)))
    # global coordinates: a moment of video 0 may lie beyond one window, and every moment lies in its video
    n = got.count.cpu().numpy()
    for p, (v, q) in enumerate(allpairs):
        assert (got.end[p, :n[p]].cpu().numpy() < (75, 40)[v]).all() and (got.start[p, :n[p]] >= 0).all()
    assert int(got.end[:3].max()) >= 32
    for name in ('window', 'start', 'end', 'score', 'prob', 'count'):
        assert torch.equal(getattr(chunked, name), getattr(got, name)), name
    assert torch.equal(by_pairs.start.cpu(), torch.from_numpy(ref_some[1])) and torch.equal(by_pairs.end.cpu(), torch.from_numpy(ref_some[2]))
    assert torch.equal(by_pairs.count.cpu(), torch.from_numpy(ref_some[5]))
    assert torch.equal(by_pairs.start[1], by_pairs.start[3]) and torch.equal(by_pairs.start[0], got.start[1 * 3 + 2])


def test_a_single_window_gives_extract_topk_on_localize():
    cfg, P, m = _model()
    video = _videos(64, (27,), seed=41)[0]
    words, chars, qmask = _queries(cfg, 3, seed=42)
    with torch.no_grad():
        wenc = m.encode_windows(video, 32, 16)
        got = m.localize_long(wenc, m.encode_query(words, chars, qmask), 5, nms_iou=0.5)
        X = torch.zeros(1, 32, 64, device='cuda')
        X[0, :27] = video
        mask = (torch.arange(32, device='cuda') < 27).float()[None]
        _, sl, el = m.localize(m.encode_video(X, mask), [0, 0, 0], words, chars, qmask)
        ref = m.extract_topk(sl, el, 5, nms_iou=0.5, lengths=[27, 27, 27])
    assert wenc.N == 1 and bool((got.window[got.start >= 0] == 0).all())
    for name in ('start', 'end', 'score', 'prob', 'count'):
        assert torch.equal(getattr(got, name), getattr(ref, name)), name


# ------------------------------------------------------------------------------------------------ 4. handles
def test_window_handles_are_checked():
    cfg, P, m = _model()
    videos = _videos(64, (75, 40), seed=51)
    q = _queries(cfg, 3, seed=52)
    with pytest.raises(RuntimeError, match='grad is enabled'):
        m.encode_windows(videos, 32, 16)
    with torch.no_grad():
        wenc, qenc = m.encode_windows(videos, 32, 16), m.encode_query(*q)
        good = m.localize_long(wenc, qenc, 3)
        out = m.localize(wenc, [0, 5, 3], *q)                     # a WindowEncoding is a VideoEncoding: localize takes it as it is
        ref = m.localize_pairs(wenc, qenc, [0, 5, 3], [0, 1, 2])
        assert all(torch.equal(a, b) for a, b in zip(out, ref))
        for bad, text in ((dict(stride=0), 'stride=0'), (dict(stride=33), 'would be skipped'), (dict(window=41, stride=8), 'max_pos_len=40')):
            with pytest.raises(ValueError, match=text):
                m.encode_windows(videos, **dict(dict(window=32, stride=16), **bad))
        with pytest.raises(ValueError, match='pairs must be'):
            m.localize_long(wenc, qenc, 3, pairs=[(2, 0)])
        with pytest.raises(TypeError, match='WindowEncoding'):
            m.localize_long(m.encode_video(torch.zeros(1, 32, 64, device='cuda'), torch.ones(1, 32, device='cuda')), qenc, 3)
    m.train()
    m.eval()
    try:
        with torch.no_grad():
            with pytest.raises(ValueError, match='stale WindowEncoding'):
                m.localize_long(wenc, qenc, 3)
            with pytest.raises(ValueError, match='stale VideoEncoding'):
                m.localize(wenc, [0], *(t[:1] for t in q))
            wenc, qenc = m.encode_windows(videos, 32, 16), m.encode_query(*q)
            assert all(torch.equal(a, b) for a, b in zip(good, m.localize_long(wenc, qenc, 3)))
            m.load_state_dict(P, strict=True)
            with pytest.raises(ValueError, match='stale'):
                m.localize_long(wenc, qenc, 3)
            eng = m._engine
            eng.has_windows = False                                  # an older library: refused by name, no fallback
            try:
                with pytest.raises(Exception, match='no sliding windows'):
                    m.encode_windows(videos, 32, 16)
            finally:
                eng.has_windows = True
    finally:
        m.eval()


def test_a_training_step_after_the_window_calls_meets_its_gate(monkeypatch):
    """One engine: a training step that meets the oracle; then encode_windows and merge_windows in its workspace -- the backward is refused there, as
    after an inference forward --; then the same step again: it meets the oracle too and leaves the bits of the first."""
    from tests.helpers import check_training_against_oracle
    from vslnet_amd import engine as E
    B, T, Lq, Lc = 4, 64, 9, 6
    real, made = E.Engine, []

    def same_engine(cfg, *a, **k):
        if not made:
            made.append(real(cfg, *a, **k))
        return made[0]
    monkeypatch.setattr(E, 'Engine', same_engine)
    step = dict(cfg=dict(video_feature_dim=64), lazy=True)
    before = check_training_against_oracle(B, T, Lq, Lc, context='before the window calls', **step)
    eng = before.eng
    feats = _videos(64, (75,), seed=61)[0]
    start, length = window_table(75, 32, 16)
    i32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.int32)).cuda()      # noqa: E731
    enc = eng.encode_windows(before.flat, feats, i32(start), i32(length), 32)
    assert enc.encoding.shape == (4, 32, 128) and bool(torch.isfinite(enc.encoding).all())
    with pytest.raises(E.VslError, match='saved nothing'):
        eng.backward(None, torch.zeros(B, T, device='cuda'), torch.zeros(B, T, device='cuda'), eng.new_flat())
    after = check_training_against_oracle(B, T, Lq, Lc, context='after the window calls', **step)
    assert len(made) == 1 and after.eng is eng and torch.equal(after.g, before.g)


# ------------------------------------------------------------------------------------------------ 5. every refusal by its message
def test_encode_windows_refusals_by_name():
    from vslnet_amd.engine import vsl_encode_windows_io
    cfg, P, m = _model()
    eng, flat = m._engine_for(torch.device('cuda')), m._flat
    feats = _videos(64, (40,), seed=71)[0]
    row, length = torch.tensor([0, 8], dtype=torch.int32, device='cuda'), torch.tensor([32, 32], dtype=torch.int32, device='cuda')
    good = eng.encode_windows(flat, feats, row, length, 32)
    n = C.c_int64()
    err = lambda: eng.lib.vsl_last_error().decode()                # noqa: E731
    for (N, T, rows), text in (((0, 32, 40), 'N=0'), ((-1, 32, 40), 'N=-1'), ((2, 0, 40), 'T=0'), ((2, 41, 40), 'T=41'), ((2, 4097, 40), 'T=4097'),
                               ((2, 32, 0), 'rows=0'), ((2, 32, 2 ** 25), 'rows * video_feature_dim'), ((2 ** 19, 32, 40), 'N * T * 128')):
        assert eng.lib.vsl_encode_windows_workspace_floats(eng.h, N, T, rows, C.byref(n)) != 0 and text in err(), ((N, T, rows), err())
    big = _model(Dv=20)[2]._engine_for(torch.device('cuda'))      # Dv 20: rows * 128 passes the limit before rows * Dv does
    assert big.lib.vsl_encode_windows_workspace_floats(big.h, 2, 32, 2 ** 24, C.byref(n)) != 0 and 'rows * 128' in big.lib.vsl_last_error().decode()
    assert eng.lib.vsl_encode_windows_workspace_floats(eng.h, 2, 32, 40, C.byref(n)) == 0
    assert n.value == eng.encode_workspace_floats(2, 32) + 40 * 128                  # the encode plan of (N, T) plus rows * 128 floats
    enc, mask = torch.empty(2, 32, 128, device='cuda'), torch.empty(2, 32, device='cuda')
    full = dict(rows=40, N=2, T=32, params=flat.data_ptr(), video_features=feats.data_ptr(), window_row=row.data_ptr(), window_len=length.data_ptr(),
                video_encoding=enc.data_ptr(), v_mask=mask.data_ptr(), workspace=eng._ws.data_ptr())
    for change, text in ((dict(params=None), 'null device pointer'), (dict(video_features=None), 'null device pointer'), (dict(video_encoding=None), 'null device pointer'),
                         (dict(v_mask=None), 'null device pointer'), (dict(workspace=None), 'null device pointer'), (dict(window_row=None), 'window_row is NULL'),
                         (dict(window_len=None), 'window_len is NULL'), (dict(N=0), 'N=0'), (dict(T=41), 'T=41'), (dict(rows=0), 'rows=0')):
        io = vsl_encode_windows_io(**dict(full, **change))
        assert eng.lib.vsl_encode_windows(eng.h, C.byref(io), None) != 0 and text in err(), (change, err())
    assert eng.lib.vsl_encode_windows(eng.h, None, None) != 0 and 'null handle' in err()
    io = vsl_encode_windows_io(**full)
    assert eng.lib.vsl_encode_windows(eng.h, C.byref(io), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert torch.equal(enc, good.encoding) and torch.equal(mask, good.v_mask)
    with pytest.raises(ValueError, match='window_row'):
        eng.encode_windows(flat, feats, row.long(), length, 32)
    with pytest.raises(ValueError, match=r'\(rows, video_feature_dim\)'):
        eng.encode_windows(flat, feats[None], row, length, 32)


def test_merge_windows_refusals_by_name():
    from vslnet_amd.engine import TopkSpans, VslError, vsl_merge_windows_io
    eng = _engine()
    lists, group, offset = _window_lists(np.random.default_rng(77), 9, 2, 3, 'random')
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    spans, dgroup, doff = TopkSpans(*(dev(x) for x in lists)), dev(group), dev(offset)
    good = eng.merge_windows(spans, dgroup, 3, 4, offset=doff)

    def again():
        assert all(torch.equal(x, y) for x, y in zip(eng.merge_windows(spans, dgroup, 3, 4, offset=doff), good))
    for kw, text in ((dict(G=0, k_out=3), 'G=0'), (dict(G=3, k_out=0), 'K_out=0'), (dict(G=3, k_out=33), 'K_out=33'), (dict(G=3, k_out=3, nms_iou=-0.1), 'nms_iou=-0.1'),
                     (dict(G=3, k_out=3, nms_iou=1.5), 'nms_iou=1.5'), (dict(G=3, k_out=3, nms_iou=float('nan')), 'nms_iou=nan')):
        with pytest.raises(VslError, match=text):
            eng.merge_windows(spans, dgroup, **kw)
        again()
    wide = TopkSpans(*(dev(np.zeros((2, 33), dtype=t)) for t in (np.int64, np.int64, np.float32, np.float32)), dev(np.zeros(2, dtype=np.int32)))
    with pytest.raises(VslError, match='K=33'):
        eng.merge_windows(wide, dev(np.zeros(2, dtype=np.int32)), 1, 1)
    none = TopkSpans(*(dev(np.zeros((0, 2), dtype=t)) for t in (np.int64, np.int64, np.float32, np.float32)), dev(np.zeros(0, dtype=np.int32)))
    with pytest.raises(VslError, match='B=0'):
        eng.merge_windows(none, dev(np.zeros(0, dtype=np.int32)), 1, 1)
    with pytest.raises(ValueError, match='offset'):
        eng.merge_windows(spans, dgroup, 3, 4, offset=doff.long())
    with pytest.raises(ValueError, match='no prob'):
        eng.merge_windows(spans._replace(prob=None), dgroup, 3, 4)
    i32, i64, f32 = (torch.zeros(64, dtype=t, device='cuda') for t in (torch.int32, torch.int64, torch.float32))
    full = dict(B=2, K=2, G=1, K_out=2, nms_iou=0.5, start=i64.data_ptr(), end=i64.data_ptr(), score=f32.data_ptr(), key=f32.data_ptr(), count=i32.data_ptr(),
                group_index=i32.data_ptr(), out_list=i32.data_ptr(), out_start=i64.data_ptr(), out_end=i64.data_ptr(), out_score=f32.data_ptr(),
                out_key=f32.data_ptr(), out_count=i32.data_ptr())
    for field, text in (('start', 'required inputs'), ('end', 'required inputs'), ('score', 'required inputs'), ('key', 'required inputs'), ('count', 'required inputs'),
                        ('group_index', 'null group_index'), ('out_list', 'required outputs'), ('out_start', 'required outputs'), ('out_end', 'required outputs'),
                        ('out_score', 'required outputs'), ('out_key', 'required outputs'), ('out_count', 'required outputs')):
        io = vsl_merge_windows_io(**{k: v for k, v in full.items() if k != field})
        assert eng.lib.vsl_merge_windows(eng.h, C.byref(io), None) != 0 and text in eng.lib.vsl_last_error().decode(), field
    assert eng.lib.vsl_merge_windows(eng.h, None, None) != 0 and 'null argument' in eng.lib.vsl_last_error().decode()
    again()
    eng.has_windows = False                                      # an older library: refused by name, no host fallback
    try:
        with pytest.raises(VslError, match='vsl_merge_windows are missing'):
            eng.merge_windows(spans, dgroup, 3, 4)
        with pytest.raises(VslError, match='no sliding windows'):
            eng.encode_windows_workspace_floats(2, 32, 40)
    finally:
        eng.has_windows = True
    again()


# ------------------------------------------------------------------------------------------------ 6. the evaluation loop
def test_eval_windows_equals_a_host_recomputation():
    from model.VSLNet import VSLNet
    from tests.test_shared_video import _shared_dataset
    from vslnet_amd import runner
    from vslnet_amd.data import ResidentSplit
    from vslnet_amd.spans import TopK
    from vslnet_amd.synthetic import make_configs
    configs = make_configs(video_feature_dim=64, max_pos_len=64, word_size=200, char_size=30, batch_size=6, drop_rate=0.2)
    recs, feats = _shared_dataset(configs, n_videos=4, per_video=3, seed=9)
    torch.manual_seed(5)
    m = VSLNet(configs, np.zeros((198, configs.word_dim), np.float32)).to('cuda').eval()
    split = ResidentSplit(recs, feats, configs, 'cuda', train=False)
    stats, text = runner.eval_windows(m, split, 'cuda', 32, 16, topk=TopK(3, 0.5, 0), pairs_per_call=7)
    assert {'window', 'window_stride', 'win_r1i3', 'win_r1i5', 'win_r1i7', 'win_mIoU', 'win_r_k_i3', 'win_r_k_i5', 'win_r_k_i7', 'win_mIoU_k'} == set(stats)
    assert text.startswith('Windows 32/16: Rank@1, IoU=0.3: ') and 'Windows 32/16: Rank@3, IoU=0.3: ' in text
    ious, best = [], []
    with torch.no_grad():
        vids = sorted(feats)
        wenc = m.encode_windows([torch.from_numpy(feats[v]).cuda() for v in vids], 32, 16)
        for a in range(0, len(recs), 6):
            idx = np.arange(a, min(len(recs), a + 6))
            Lq, Lc = int(split.nwords[idx].max()), int(split.nchars[idx].max())
            words, chars = split.d_words[idx[0]:idx[-1] + 1, :Lq].contiguous(), split.d_chars[idx[0]:idx[-1] + 1, :Lq, :Lc].contiguous()
            got = m.localize_long(wenc, m.encode_query(words, chars, (words != 0).float()), 3, nms_iou=0.5, pairs=[(split.vid_of[i], q) for q, i in enumerate(idx)])
            s, e, c = got.start.cpu().numpy(), got.end.cpu().numpy(), got.count.cpu().numpy()
            for q, i in enumerate(idx):
                assert c[q] >= 1 and e[q, :c[q]].max() < recs[i]['v_len']
                ious.append(runner.best_iou_of_spans(s[q], e[q], 1, recs[i]))
                best.append(runner.best_iou_of_spans(s[q], e[q], c[q], recs[i]))
    want, _ = runner.summarise_windows(ious, best, 32, 16, TopK(3, 0.5, 0))
    assert stats == want, (stats, want)
    assert stats['win_r_k_i5'] >= stats['win_r1i5'] and stats['win_mIoU_k'] >= stats['win_mIoU']
    plain, _ = runner.eval_windows(m, split, 'cuda', 32, 16)
    assert set(plain) == {'window', 'window_stride', 'win_r1i3', 'win_r1i5', 'win_r1i7', 'win_mIoU'}
