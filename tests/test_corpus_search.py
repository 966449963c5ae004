"""Searching a collection of videos: vsl_encode_query (one encoding per query), vsl_localize_pairs (pairs of resident encodings: no query branch),
vsl_merge_topk (the device-side merge that turns per-(query, video) top-K lists into one ranked list per query), and what is built on them:
Engine / VSLNet.encode_query, localize_pairs, merge_topk, VSLNet.retrieve, runner.eval_corpus, main.py --corpus.

CPU: the exports and the ABI (version 9, vsl_io / vsl_localize_io where they were, the ctypes mirrors of the three new structs), the oracle restatement
"encode the queries once, index_select both sides, the rest", and the merge's specification (vslnet_amd.spans.merge_topk_reference): the order rule on
hand-made ties, count and fill values, the two-level property on keys drawn from 8 values so that ties dominate.
GPU: the query encoding against the saved path's `qenc`; localize_pairs against localize on the replicated queries at every dispatch boundary of the
CQ stage; the reference's goldens; workspace bounds; the launch ledgers; the merge kernel against its specification, bit for bit on every output;
retrieve against a host recomputation; misuse by name; a training step around the new calls; eval_corpus and the CLI.

Finding of the bit-equality run (MI355X).  localize_pairs has the BITS of localize on the replicated queries at every shape whose query encoding does not
depend on the query's position in its batch: the sample-local k_query_fwd (8 heads, Lq <= 32: T 24 / 128 / 160 / 117, and the rnn head) and whole-tile
Lq; 4 heads at Lq 9 came out bit-equal too.  At Lq 33, 70 and 100 (row-tile query path, Lq off the 32-row tile) the outputs differ from localize by at
most 1.3e-6 (h_score) and 6.7e-6 (logits; gates 2e-5 and 3.3e-4 .. 9.5e-4) -- NOT because of the indexed CQ kernels: localize encodes query q at batch
position b, encode_query at position q, and an EXISTING kernel rounds a row by its position.  Located with saved-path forwards alone, the same query
at two batch positions, tap by tap: emb_concat, embedding_net and qenc_x0 are bit-equal, qenc_y0 -- the output of conv layer 0 of the query pass -- is
the first tap that differs (2.4e-7 .. 4.8e-7 in 64 / 176 / 192 rows at Lq 33 / 70 / 100, 1.3e-6 in the encoder's output); at Lq 64 and at 4 heads with
Lq 9 every tap is bit-equal.  That is k_convblock_fwd's depthwise convolution on tiles that cross a sample boundary, the finding
tests/test_shared_video.py records for T off the tile.  Those cases are gated at the golden tolerances (position_free() below says which), as DESIGN
section 7 records; the query encoding itself always equals the saved `qenc` of the same Q queries."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import ROOT, header_fields, header_sizeof
from vslnet_amd.spans import merge_topk_reference

NEW_SYMBOLS = ('vsl_merge_topk', 'vsl_encode_query_workspace_floats', 'vsl_encode_query', 'vsl_pairs_workspace_floats', 'vsl_localize_pairs')
PARENT_SIZEOF_VSL_IO = 208               # sizeof(vsl_io) of the commit this feature was added to (ABI 9, `inference` last): the struct must not move
PARENT_SIZEOF_VSL_LOCALIZE_IO = 128      # ... and sizeof(vsl_localize_io) there (`workspace` last)
PARENT_LOCALIZE_FIELDS = ['B', 'T', 'Lq', 'Lc', 'N', 'params', 'pad_vec', 'glove_vec', 'word_ids', 'char_ids', 'q_mask', 'video_encoding', 'v_mask',
                          'video_index', 'h_score', 'start_logits', 'end_logits', 'workspace']


# ------------------------------------------------------------------------------------------------ 1. the ABI (CPU)
def _header():
    return open(os.path.join(ROOT, 'include', 'vslnet_hip.h')).read()


def test_library_exports_the_merge_and_keeps_abi_9():
    from vslnet_amd import build, engine
    lib = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in engine.ABI_SYMBOLS, s
    assert lib.vsl_abi_version() == 9 == engine.ABI_VERSION
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', _header())
    # (the mirrors of vsl_merge_io, vsl_encode_query_io and vsl_pairs_io against the header and the host compiler: tests/test_abi_layout.py, as for
    # every struct)
    assert ctypes.sizeof(engine.vsl_io) == header_sizeof('vsl_io') == PARENT_SIZEOF_VSL_IO and header_fields('vsl_io')[-1] == 'inference'
    assert ctypes.sizeof(engine.vsl_localize_io) == header_sizeof('vsl_localize_io') == PARENT_SIZEOF_VSL_LOCALIZE_IO
    assert header_fields('vsl_localize_io') == PARENT_LOCALIZE_FIELDS == [f[0] for f in engine.vsl_localize_io._fields_]


# ------------------------------------------------------------------------------------------------ 2. the specification (CPU)
def _lists(rng, B, K, quantised=True, empty=0.1):
    """B candidate lists of K slots as extract_topk leaves them: count[b] filled slots, the fill values behind them.  quantised: keys drawn from 8
    values, so that ties dominate; otherwise distinct-looking uniform keys."""
    count = rng.integers(1, K + 1, B).astype(np.int32)
    count[rng.random(B) < empty] = 0
    start = rng.integers(0, 50, (B, K)).astype(np.int64)
    end = start + rng.integers(0, 20, (B, K))
    score = (3.0 * rng.standard_normal((B, K))).astype(np.float32)
    key = (rng.integers(0, 8, (B, K)) / 8.0).astype(np.float32) if quantised else rng.random((B, K)).astype(np.float32)
    fill = np.arange(K)[None, :] >= count[:, None]
    start[fill], end[fill], score[fill], key[fill] = -1, -1, -np.inf, 0.0
    return start, end, score, key, count


def test_the_order_rule_on_hand_made_ties():
    #         list 0           list 1           list 2 (other group)   list 3
    key = np.array([[0.5, 0.5], [0.5, 0.9], [0.9, 0.9], [0.5, 0.25]], dtype=np.float32)
    start = np.arange(8, dtype=np.int64).reshape(4, 2)
    end, score = start + 10, np.arange(8, dtype=np.float32).reshape(4, 2) - 3
    count, group = np.array([2, 2, 2, 1], dtype=np.int32), np.array([0, 0, 1, 0], dtype=np.int32)
    tag, lst, s, e, sc, k, c = merge_topk_reference(start, end, score, key, count, group, 2, 8)
    # group 0, tag = list: 0.9 of list 1; then the 0.5 s by list, then slot; list 3's second slot is beyond its count
    assert c.tolist() == [5, 2]
    assert lst[0, :5].tolist() == [1, 0, 0, 1, 3] and s[0, :5].tolist() == [3, 0, 1, 2, 6] and tag[0, :5].tolist() == [1, 0, 0, 1, 3]
    assert e[0, :5].tolist() == [13, 10, 11, 12, 16] and sc[0, :5].tolist() == [0.0, -3.0, -2.0, -1.0, 3.0]
    assert np.array_equal(k[0, :5], np.array([0.9, 0.5, 0.5, 0.5, 0.5], dtype=np.float32))
    assert lst[1, :2].tolist() == [2, 2] and s[1, :2].tolist() == [4, 5]
    # the fill values
    assert (tag[0, 5:] == -1).all() and (lst[0, 5:] == -1).all() and (s[0, 5:] == -1).all() and (e[0, 5:] == -1).all()
    assert np.isneginf(sc[0, 5:]).all() and (k[0, 5:] == 0).all()
    assert (tag.dtype, lst.dtype, s.dtype, e.dtype, sc.dtype, k.dtype, c.dtype) == (np.int32, np.int32, np.int64, np.int64, np.float32, np.float32, np.int32)
    # a tag per list goes in front of the list number: list 3 (tag 0) now leads the 0.5 s, list 0 (tag 7) closes them
    tag, lst, s = merge_topk_reference(start, end, score, key, count, group, 2, 8, tag=np.array([7, 5, 0, 0], dtype=np.int32))[:3]
    assert lst[0, :5].tolist() == [1, 3, 1, 0, 0] and tag[0, :5].tolist() == [5, 0, 5, 7, 7] and s[0, :5].tolist() == [3, 6, 2, 0, 1]
    # a tag per slot
    per_slot = np.array([[3, 1], [2, 9], [0, 0], [1, 0]], dtype=np.int32)
    tag, lst, s = merge_topk_reference(start, end, score, key, count, group, 2, 3, tag=per_slot)[:3]
    assert tag[0].tolist() == [9, 1, 1] and lst[0].tolist() == [1, 0, 3] and s[0].tolist() == [3, 1, 6]      # k_out cuts the list
    # no group at all
    out = merge_topk_reference(start, end, score, key, count, np.array([-1, 2, 9, 2 ** 31 - 1], dtype=np.int32), 2, 4)
    assert out[6].tolist() == [0, 0] and (out[0] == -1).all() and np.isneginf(out[4]).all()


def _chunked(merge, lists, group, tags, G, k_out, chunks, k_chunk):
    """two levels: `merge` over each chunk of lists, then over the chunks' results with their tags carried per slot"""
    start, end, score, key, count = lists
    first = [merge(start[a:b], end[a:b], score[a:b], key[a:b], count[a:b], group[a:b], G, k_chunk, tags[a:b]) for a, b in chunks]
    cat = lambda i: np.concatenate([f[i] for f in first])      # noqa: E731
    return merge(cat(2), cat(3), cat(4), cat(5), cat(6), np.tile(np.arange(G, dtype=np.int32), len(chunks)), G, k_out, cat(0))


def _two_level_case(seed):
    rng = np.random.default_rng(seed)
    B, K, G = int(rng.integers(20, 80)), int(rng.integers(1, 7)), int(rng.integers(1, 5))
    lists = _lists(rng, B, K)
    group = rng.integers(-1, G + 1, B).astype(np.int32)         # (-1 and G: in no group)
    cuts = sorted(set([0, B] + rng.integers(1, B, 3).tolist()))
    chunks = list(zip(cuts[:-1], cuts[1:]))
    # every tag lives in exactly one chunk; inside a chunk several lists share one
    tags = np.concatenate([1000 * i + rng.integers(0, 3, b - a) for i, (a, b) in enumerate(chunks)]).astype(np.int32)
    k_out = int(rng.integers(1, 9))
    return lists, group, tags, G, k_out, chunks, k_out + int(rng.integers(0, 3))


def test_two_levels_give_the_one_level_result():
    for seed in range(40):
        lists, group, tags, G, k_out, chunks, k_chunk = _two_level_case(seed)
        one = merge_topk_reference(*lists, group, G, k_out, tags)
        two = _chunked(merge_topk_reference, lists, group, tags, G, k_out, chunks, k_chunk)
        for i in (0, 2, 3, 4, 5, 6):                              # (`list` numbers the second level's rows)
            assert np.array_equal(one[i].view(np.int32) if one[i].dtype == np.float32 else one[i],
                                  two[i].view(np.int32) if two[i].dtype == np.float32 else two[i]), (seed, i)


# ------------------------------------------------------------------------------------------------ 3. the kernel against the specification (GPU)
@functools.lru_cache(maxsize=None)
def _engine():
    from vslnet_amd.engine import Engine
    return Engine(O.make_cfg(video_feature_dim=64, max_pos_len=32, word_size=52))


def _device_merge(start, end, score, key, count, group, G, k_out, tag=None):
    """Engine.merge_topk on host arrays -> the specification's tuple of numpy arrays"""
    from vslnet_amd.engine import TopkSpans
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    m = _engine().merge_topk(TopkSpans(dev(start), dev(end), dev(score), dev(key), dev(count)), dev(group), G, k_out, tag=None if tag is None else dev(tag))
    assert (m.tag.dtype, m.list.dtype, m.start.dtype, m.end.dtype, m.score.dtype, m.prob.dtype, m.count.dtype) == \
        (torch.int32, torch.int32, torch.int64, torch.int64, torch.float32, torch.float32, torch.int32)
    return tuple(x.cpu().numpy() for x in m)


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _assert_same(got, ref, context, skip=()):
    for i, name in enumerate(('tag', 'list', 'start', 'end', 'score', 'key', 'count')):
        if name not in skip:
            assert got[i].shape == ref[i].shape and np.array_equal(_bits(got[i]), _bits(ref[i])), (context, name, got[i], ref[i])


#              B   K  G  K_out quantised  group            tag
MERGE_CASES = [(1, 1, 1, 1, False, 'all', None),                # the smallest call
               (300, 5, 3, 10, False, 'random', 'list'),        # lists above the 256-thread stride
               (300, 5, 3, 10, True, 'random', None),           # ... with massive ties, tag NULL
               (3, 4, 1, 32, False, 'all', 'list'),             # exhaustion: fewer candidates than K_out
               (40, 32, 2, 32, True, 'random', 'slot'),         # both limits, a tag per slot
               (64, 5, 4, 5, True, 'holes', 'list'),            # an empty group and lists in no group
               (700, 3, 1, 7, True, 'all', 'shared'),           # one group, three strides, tags shared by several lists
               (9, 2, 5, 3, False, 'random', None)]


def _merge_case(case):
    B, K, G, k_out, quantised, how, tagkind = MERGE_CASES[case]
    rng = np.random.default_rng(9000 + case)
    lists = _lists(rng, B, K, quantised=quantised, empty=0.0 if B < 4 else 0.15)
    if how == 'all':
        group = np.zeros(B, dtype=np.int32)
    elif how == 'random':
        group = rng.integers(0, G, B).astype(np.int32)
    else:                                                        # group 1 stays empty; -1, G and the largest int are no group
        group = rng.choice(np.array([0, 2, 3, -1, G, 2 ** 31 - 1, -2 ** 31]), B).astype(np.int32)
    tag = {None: None, 'list': rng.permutation(B).astype(np.int32), 'shared': rng.integers(0, 4, B).astype(np.int32),
           'slot': rng.integers(0, 6, (B, K)).astype(np.int32)}[tagkind]
    return lists, group, G, k_out, tag


@pytest.mark.gpu
@pytest.mark.parametrize('case', range(len(MERGE_CASES)))
def test_merge_equals_the_specification_bit_for_bit(case):
    lists, group, G, k_out, tag = _merge_case(case)
    ref = merge_topk_reference(*lists, group, G, k_out, tag)
    _assert_same(_device_merge(*lists, group, G, k_out, tag), ref, MERGE_CASES[case])
    if MERGE_CASES[case][5] == 'holes':
        assert ref[6][1] == 0 and (ref[6] > 0).any()            # the empty group is empty, another is not
    if MERGE_CASES[case][3] == 32 and MERGE_CASES[case][0] == 3:
        assert 0 < ref[6][0] < 32                               # exhaustion


def test_the_merge_cases_cover_what_they_must():
    assert (1, 1, 1, 1) in {c[:4] for c in MERGE_CASES} and (300, 5, 3, 10) in {c[:4] for c in MERGE_CASES}
    assert {c[6] for c in MERGE_CASES} == {None, 'list', 'slot', 'shared'} and {c[5] for c in MERGE_CASES} == {'all', 'random', 'holes'}
    assert any(c[0] > 512 for c in MERGE_CASES) and any(c[1] == 32 and c[3] == 32 for c in MERGE_CASES) and any(c[4] for c in MERGE_CASES)
    lists = _merge_case(1)[0]
    assert (lists[4] == 0).any()                                 # lists with count 0


@pytest.mark.gpu
def test_two_levels_give_the_one_level_result_on_the_device():
    for seed in (3, 17, 31):
        lists, group, tags, G, k_out, chunks, k_chunk = _two_level_case(seed)
        one = _device_merge(*lists, group, G, k_out, tags)
        _assert_same(one, merge_topk_reference(*lists, group, G, k_out, tags), ('one level', seed))
        _assert_same(_chunked(_device_merge, lists, group, tags, G, k_out, chunks, k_chunk), one, ('two levels', seed), skip=('list',))


@pytest.mark.gpu
def test_two_merges_and_a_side_stream_give_the_same_bits():
    from vslnet_amd.engine import TopkSpans
    lists, group, G, k_out, tag = _merge_case(2)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    spans, dgroup = TopkSpans(*(dev(x) for x in lists)), dev(group)
    eng = _engine()
    a = eng.merge_topk(spans, dgroup, G, k_out)
    b = eng.merge_topk(spans, dgroup, G, k_out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = eng.merge_topk(spans, dgroup, G, k_out)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.gpu
def test_merge_misuse_is_refused_by_name_and_the_next_call_works():
    from vslnet_amd.engine import TopkSpans, VslError
    eng = _engine()
    lists, group, G, k_out, _ = _merge_case(7)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    spans, dgroup = TopkSpans(*(dev(x) for x in lists)), dev(group)
    good = eng.merge_topk(spans, dgroup, G, k_out)

    def again():
        assert all(torch.equal(x, y) for x, y in zip(eng.merge_topk(spans, dgroup, G, k_out), good))
    for kw, text in ((dict(G=0, k_out=3), 'G=0'), (dict(G=-1, k_out=3), 'G=-1'), (dict(G=G, k_out=0), 'K_out=0'), (dict(G=G, k_out=33), 'K_out=33')):
        with pytest.raises(VslError, match=text):
            eng.merge_topk(spans, dgroup, **kw)
        again()
    wide = TopkSpans(*(dev(np.zeros((2, 33), dtype=t)) for t in (np.int64, np.int64, np.float32, np.float32)), dev(np.zeros(2, dtype=np.int32)))
    with pytest.raises(VslError, match='K=33'):
        eng.merge_topk(wide, dev(np.zeros(2, dtype=np.int32)), 1, 1)
    none = TopkSpans(*(dev(np.zeros((0, 2), dtype=t)) for t in (np.int64, np.int64, np.float32, np.float32)), dev(np.zeros(0, dtype=np.int32)))
    with pytest.raises(VslError, match='B=0'):
        eng.merge_topk(none, dev(np.zeros(0, dtype=np.int32)), 1, 1)
    again()
    with pytest.raises(ValueError, match='not a C int'):
        eng.merge_topk(spans, dgroup, 2 ** 32 + 1, k_out)
    with pytest.raises(ValueError, match='no prob'):
        eng.merge_topk(spans._replace(prob=None), dgroup, G, k_out)
    with pytest.raises(ValueError, match='group_index'):
        eng.merge_topk(spans, dgroup.long(), G, k_out)
    with pytest.raises(ValueError, match='spans.count'):
        eng.merge_topk(spans._replace(count=spans.count.long()), dgroup, G, k_out)
    with pytest.raises(ValueError, match='tag'):
        eng.merge_topk(spans, dgroup, G, k_out, tag=dgroup[:-1].contiguous())
    again()
    # the raw entry point: every required pointer is checked by name
    from vslnet_amd.engine import vsl_merge_io
    i32, i64, f32 = (torch.zeros(64, dtype=t, device='cuda') for t in (torch.int32, torch.int64, torch.float32))
    full = dict(B=2, K=2, G=1, K_out=2, start=i64.data_ptr(), end=i64.data_ptr(), score=f32.data_ptr(), key=f32.data_ptr(), count=i32.data_ptr(),
                group_index=i32.data_ptr(), out_tag=i32.data_ptr(), out_list=i32.data_ptr(), out_start=i64.data_ptr(), out_end=i64.data_ptr(),
                out_score=f32.data_ptr(), out_key=f32.data_ptr(), out_count=i32.data_ptr())
    for field, text in (('start', 'required inputs'), ('key', 'required inputs'), ('count', 'required inputs'), ('group_index', 'null group_index'),
                        ('out_tag', 'required outputs'), ('out_count', 'required outputs')):
        io = vsl_merge_io(**{k: v for k, v in full.items() if k != field})
        assert eng.lib.vsl_merge_topk(eng.h, ctypes.byref(io), None) != 0 and text in eng.lib.vsl_last_error().decode()
    io = vsl_merge_io(tag_per_slot=1, **full)
    assert eng.lib.vsl_merge_topk(eng.h, ctypes.byref(io), None) != 0 and 'tag_per_slot' in eng.lib.vsl_last_error().decode()
    again()
    eng.has_merge_topk = False                                   # an older library: refused by name, no host fallback
    try:
        with pytest.raises(VslError, match='vsl_merge_topk is missing'):
            eng.merge_topk(spans, dgroup, G, k_out)
    finally:
        eng.has_merge_topk = True
    again()


@pytest.mark.gpu
def test_merge_is_legal_after_any_forward_and_on_extract_topk_output():
    """the lists of a real search: localize 3 queries against 2 videos each way, extract_topk, merge per query; the result is the specification's on the
    device's own lists, and its tags are videos"""
    eng = _engine()
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=32, word_size=52)
    P = O.random_params(cfg, seed=21)
    from vslnet_amd.engine import flat_from_state_dict
    flat = flat_from_state_dict(eng, P)
    vb = O.synthetic_batch(cfg, 2, 24, 7, 6, seed=22, ragged=True)
    qb = O.synthetic_batch(cfg, 3, 24, 7, 6, seed=23, ragged=True)
    enc = eng.encode_video(flat, vb['vfeats'].cuda(), vb['v_mask'].cuda())
    q, v = [0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1]
    _, sl, el = eng.localize(flat, P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda(), enc, v,
                             qb['word_ids'][q].cuda(), qb['char_ids'][q].cuda(), qb['q_mask'][q].cuda())
    spans = eng.extract_topk(sl, el, 4, nms_iou=0.5, v_mask=vb['v_mask'][v].cuda())
    group, tag = torch.tensor(q, dtype=torch.int32, device='cuda'), torch.tensor(v, dtype=torch.int32, device='cuda')
    m = eng.merge_topk(spans, group, 3, 5, tag=tag)
    ref = merge_topk_reference(*(x.cpu().numpy() for x in spans[:3]), spans.prob.cpu().numpy(), spans.count.cpu().numpy(), np.array(q), 3, 5, np.array(v))
    _assert_same(tuple(x.cpu().numpy() for x in m), ref, 'after localize')
    assert (m.count.cpu() == 5).all() and set(m.tag.cpu().reshape(-1).tolist()) <= {0, 1}
    p = m.prob.cpu()
    assert (p[:, :-1] >= p[:, 1:]).all()


# ------------------------------------------------------------------------------------------------ 4. the oracle, restated for both sides (CPU)
def oracle_pairs(P, cfg, vfeats, v_mask, vidx, word_ids, char_ids, q_mask, qidx):
    """O.forward with BOTH halves hoisted: the N videos and the Q queries go through their branches ONCE, the two encodings and their masks are
    index_select-ed per pair, everything else is O.forward's own sequence.  The oracle itself is not edited."""
    p, H = float(cfg.drop_rate), int(cfg.num_heads)
    venc = O.feature_encoder(P, 'feature_encoder.', O.visual_projection(P, vfeats, p, False), v_mask, H, p, False, None)
    qenc = O.feature_encoder(P, 'feature_encoder.', O.embedding(P, word_ids, char_ids, p, False), q_mask, H, p, False, None)
    vidx, qidx = torch.as_tensor(vidx, dtype=torch.int64), torch.as_tensor(qidx, dtype=torch.int64)
    ve, vm = torch.index_select(venc, 0, vidx), torch.index_select(v_mask, 0, vidx)
    qe, qm = torch.index_select(qenc, 0, qidx), torch.index_select(q_mask, 0, qidx)
    f1 = O.cq_attention(P, ve, qe, vm, qm, p, False, None)
    f2 = O.cq_concat(P, f1, qe, qm)
    h = O.highlight(P, f2, vm)
    sl, el = O.conditioned_predictor(P, f2 * h[:, :, None], vm, cfg.predictor, H, p, False, None)
    return h, sl, el


def test_oracle_restatement_of_pairs_equals_the_forward_on_the_replicated_batch():
    from tests.test_shared_video import _videos_and_queries
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=64, word_size=102)
    P = O.random_params(cfg, seed=11)
    vidx, qidx = [0, 0, 2, 1, 0, 2, 2], [3, 0, 0, 1, 3, 3, 1]
    vb, qb = _videos_and_queries(cfg, 3, 4, 64, 9, 6, seed=12)
    with torch.no_grad():
        h, sl, el = oracle_pairs(P, cfg, vb['vfeats'], vb['v_mask'], vidx, qb['word_ids'], qb['char_ids'], qb['q_mask'], qidx)
        rh, rsl, rel = O.forward(P, cfg, qb['word_ids'][qidx], qb['char_ids'][qidx], vb['vfeats'][vidx], vb['v_mask'][vidx], qb['q_mask'][qidx])
    for nm, a, c in (('h_score', h, rh), ('start_logits', sl, rsl), ('end_logits', el, rel)):
        assert torch.equal(a, c), '%s: max |diff| %g' % (nm, float((a - c).abs().max()))


# ------------------------------------------------------------------------------------------------ 5. the query encoding (GPU)
def _row(N, Q, T, Lq, heads=8, predictor='transformer', word_table=False, extreme=False):
    """the case dict of tests.test_shared_video._setup: N videos, Q queries drawn independently"""
    return dict(N=N, B=Q, idx=None, T=T, Lq=Lq, heads=heads, predictor=predictor, Dv=64, ragged=True, extreme=extreme, bf16=False, word_table=word_table, Lc=6)


def _query_pass_labels(heads, Lq):
    """launches of the query branch (forward.hip query_branch)"""
    if heads == 8 and Lq <= 32:
        return ['embed_fwd', 'query_fwd']
    return ['embed_fwd', 'linear_fwd', 'convblock_fwd'] + (['attn_block_fwd'] if heads == 8 and Lq <= 128 else ['attn_fwd', 'attn_out_fwd'])


ENCODE_CASES = [pytest.param(8, 9, False, id='H8-Lq9'), pytest.param(8, 32, False, id='H8-Lq32'), pytest.param(8, 33, False, id='H8-Lq33'),
                pytest.param(8, 70, False, id='H8-Lq70'), pytest.param(8, 100, False, id='H8-Lq100'), pytest.param(4, 9, False, id='H4-Lq9'),
                pytest.param(8, 9, True, id='word-table-Lq9')]


@pytest.mark.gpu
@pytest.mark.parametrize('heads,Lq,word_table', ENCODE_CASES)
def test_query_encoding_equals_the_saved_paths_qenc(heads, Lq, word_table):
    from collections import Counter
    from tests.test_shared_video import _ledger, _setup
    Q, T = 5, 32
    cfg, P, vb, qb, dv, dq, eng, flat, pg = _setup(_row(Q, Q, T, Lq, heads=heads, word_table=word_table, extreme=True))
    assert eng.has_query_encoding and eng.has_merge_topk
    qenc, names = _ledger(eng, lambda: eng.encode_query(flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dq['q_mask']))
    assert (qenc.Q, qenc.Lq, qenc.Lc) == (Q, Lq, 6) and qenc.encoding.shape == (Q, Lq, 128) and qenc.q_mask is dq['q_mask']
    # the ledger: two packs and the query branch, nothing of the video side or behind the join
    print('[ledger] H %d Lq %d: encode_query %s' % (heads, Lq, names))
    assert Counter(names) == Counter(['pack', 'pack'] + _query_pass_labels(heads, Lq)), names
    assert not [n for n in names if n.startswith('cq_') or n in ('vproj_fwd', 'head_fwd', 'lstm_fwd', 'rnn_fwd', 'lstm_gi', 'vmask_gather')], names
    # the workspace: never more than the inference plan of (Q, T = 32, Lq, Lc)
    n_q, n_inf = eng.encode_query_workspace_floats(Q, Lq, 6), eng.inference_workspace_floats(Q, 32, Lq, 6)
    print('[workspace] H %d Lq %d: encode_query %d / inference(T = 32) %d floats = %.4f' % (heads, Lq, n_q, n_inf, n_q / n_inf))
    assert n_q <= n_inf
    # nothing saved: the saved path's taps and the backward are refused until a saved-path forward has run
    from vslnet_amd.engine import VslError
    with pytest.raises(VslError, match='saves nothing'):
        eng.ws_view('qenc', (Q, Lq, 128))
    assert eng.lib.vsl_workspace_offset(eng.h, Q, T, Lq, 6, b'qenc') == -2 and b'saved nothing' in eng.lib.vsl_last_error()
    kept = qenc.encoding.clone()
    eng.forward(flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dv['vfeats'], dv['v_mask'], dq['q_mask'], training=False)
    saved = eng.ws_view('qenc', (Q, Lq, 128))
    assert torch.equal(kept, saved), 'H %d Lq %d: the encoding differs from the saved qenc, max |diff| %g' % (heads, Lq, float((kept - saved).abs().max()))
    assert torch.equal(kept, eng.encode_query(flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dq['q_mask']).encoding)


# ------------------------------------------------------------------------------------------------ 6. pairs against localize on the replicated queries (GPU)
#              id                          T    Lq  heads predictor
PAIR_SHAPES = [('T24-Lq9', 24, 9, 8, 'transformer'), ('T128-Lq32-fold-edge', 128, 32, 8, 'transformer'), ('T160-Lq9-cq-col', 160, 9, 8, 'transformer'),
               ('T64-Lq33-row-tile-query', 64, 33, 8, 'transformer'), ('T64-Lq70-score12', 64, 70, 8, 'transformer'),
               ('T64-Lq100-score16', 64, 100, 8, 'transformer'), ('T117-Lq9-off-tile', 117, 9, 8, 'transformer'), ('H4-T64-Lq9', 64, 9, 4, 'transformer'),
               ('rnn-T64-Lq9', 64, 9, 8, 'rnn')]
# indices over N = 5 videos and Q = 8 queries (videos 1, 3 and queries 2, 4, 7 unused; repeats on both sides), then Q = 1 with B = 8 and Q = 8 with B = 1
PAIR_INDICES = [('repeated-unused', 8, [0, 0, 2, 4, 0, 2, 2], [6, 0, 0, 1, 6, 3, 5]), ('Q1-B8', 1, [0, 1, 2, 3, 4, 4, 0, 2], [0] * 8), ('Q8-B1', 8, [3], [5])]


def position_free(heads, Lq):
    """Is the query encoding independent of the query's position in its batch?  The sample-local k_query_fwd (8 heads, Lq <= 32), or rows that fill
    whole 32-row tiles.  These cases are gated bit for bit without exception; the others take the golden tolerances when the run finds a difference."""
    return (heads == 8 and Lq <= 32) or Lq % 32 == 0


def test_the_pair_cases_cover_what_they_must():
    assert {(s[1], s[2]) for s in PAIR_SHAPES} == {(24, 9), (128, 32), (160, 9), (64, 33), (64, 70), (64, 100), (117, 9), (64, 9)}
    assert any(s[3] == 4 for s in PAIR_SHAPES) and any(s[4] == 'rnn' for s in PAIR_SHAPES)
    free = [s for s in PAIR_SHAPES if position_free(s[3], s[2])]
    assert all(s in free for s in PAIR_SHAPES if s[3] == 8 and s[2] <= 32) and len(free) >= 5       # at most 4 of the 9 shapes may take the tolerance gate
    assert {s[2] for s in PAIR_SHAPES if not position_free(s[3], s[2])} == {33, 70, 100, 9} and [s for s in PAIR_SHAPES if s[3] == 4][0] not in free
    assert {(i[1], len(i[2])) for i in PAIR_INDICES} == {(8, 7), (1, 8), (8, 1)}
    _, _, vidx, qidx = PAIR_INDICES[0]
    assert len(set(vidx)) < 5 and len(set(qidx)) < 8 and len(set(vidx)) < len(vidx) and len(set(qidx)) < len(qidx)      # repeated AND unused, both sides


@pytest.mark.gpu
@pytest.mark.parametrize('shape', PAIR_SHAPES, ids=[s[0] for s in PAIR_SHAPES])
def test_pairs_equal_localize_on_the_replicated_queries(shape):
    from collections import Counter
    from tests.test_shared_video import _gate, _ledger, _setup
    cid, T, Lq, heads, predictor = shape
    N = 5
    for extreme in (False, True):                                # extreme: query 0 has ONE word, the last video ONE clip
        cfg, P, vb, qb, dv, dq, eng, flat, pg = _setup(_row(N, 8, T, Lq, heads=heads, predictor=predictor, extreme=extreme))
        venc = eng.encode_video(flat, dv['vfeats'], dv['v_mask'])
        for iname, Q, vidx, qidx in (PAIR_INDICES[:1] if extreme else PAIR_INDICES):
            ctx = '%s %s%s' % (cid, iname, ' extreme' if extreme else '')
            words, chars, qmask = (dq[k][:Q].contiguous() for k in ('word_ids', 'char_ids', 'q_mask'))
            qenc = eng.encode_query(flat, pg[0], pg[1], words, chars, qmask)
            B = len(vidx)
            n_pairs, n_loc = eng.pairs_workspace_floats(B, T, Lq), eng.localize_workspace_floats(B, T, Lq, 6)
            print('[workspace] %s: pairs %d / localize %d floats = %.4f' % (ctx, n_pairs, n_loc, n_pairs / n_loc))
            assert n_pairs <= n_loc
            got, names = _ledger(eng, lambda: [t.clone() for t in eng.localize_pairs(flat, venc, qenc, vidx, qidx)])
            dq_idx = torch.tensor(qidx).cuda()
            rep = [t.index_select(0, dq_idx).contiguous() for t in (words, chars, qmask)]
            ref, names_loc = _ledger(eng, lambda: [t.clone() for t in eng.localize(flat, pg[0], pg[1], venc, vidx, *rep)])
            # the ledger: what localize launches minus the whole query branch; one pack instead of its three
            print('[ledger] %s: localize_pairs %s' % (ctx, names))
            assert not [n for n in names if n in ('embed_fwd', 'query_fwd', 'linear_fwd', 'vproj_fwd')] and names.count('vmask_gather') == 1, (ctx, names)
            strip = lambda c: Counter({k: v for k, v in c.items() if k != 'pack'})      # noqa: E731
            assert strip(Counter(names)) == strip(Counter(names_loc) - Counter(_query_pass_labels(heads, Lq))), (ctx, names, names_loc)
            assert names.count('pack') == 1
            padm = (dv['v_mask'][torch.tensor(vidx).cuda()] == 0)
            same = all(torch.equal(a, c) for a, c in zip(got, ref))
            diff = [float((a - c)[~padm].abs().max()) for a, c in zip(got, ref)]
            print('[pairs] %s: bit-equal to localize on the replicated queries: %s ; max |diff| h_score %.3g start %.3g end %.3g' % (ctx, same, *diff))
            if position_free(heads, Lq):
                for nm, a, c in zip(('h_score', 'start_logits', 'end_logits'), got, ref):
                    assert torch.equal(a, c), '%s: %s differs from localize, max |diff| %g' % (ctx, nm, float((a - c).abs().max()))
            else:
                gn, rn = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in ref]
                _gate(ctx, gn[0], gn[1], gn[2], rn[0], rn[1], rn[2], padm.cpu().numpy())
            si, ei = eng.extract_index(got[1], got[2])
            sr, er = eng.extract_index(ref[1], ref[2])
            assert torch.equal(si, sr) and torch.equal(ei, er), ctx
            assert bool((got[1][padm] == -1e30).all()) and bool((got[2][padm] == -1e30).all()) and bool((got[0][padm] == 0).all()), ctx
            # device indices are taken as they are: same bits
            again = eng.localize_pairs(flat, venc, qenc, torch.tensor(vidx).cuda(), dq_idx.to(torch.int32))
            assert all(torch.equal(a, c) for a, c in zip(got, again)), ctx


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny_tf', 'tiny_rnn'])
def test_pairs_match_the_reference_goldens(name):
    from tests.helpers import load_golden
    from tests.test_shared_video import _gate
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg, P, b, z = load_golden(name)
    eng = Engine(cfg)
    flat = flat_from_state_dict(eng, P)
    d = {k: v.cuda().contiguous() for k, v in b.items()}
    B = d['vfeats'].shape[0]
    venc = eng.encode_video(flat, d['vfeats'], d['v_mask'])
    qenc = eng.encode_query(flat, P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda(), d['word_ids'], d['char_ids'], d['q_mask'])
    h, sl, el = (t.cpu().numpy() for t in eng.localize_pairs(flat, venc, qenc, np.arange(B), np.arange(B)))
    _gate(name, h, sl, el, z['out.h_score'], z['out.start_logits'], z['out.end_logits'], b['v_mask'].numpy() == 0)
    si, ei = eng.extract_index(torch.from_numpy(sl).cuda(), torch.from_numpy(el).cuda())
    assert np.array_equal(si.cpu().numpy(), z['out.start_index']) and np.array_equal(ei.cpu().numpy(), z['out.end_index'])


# ------------------------------------------------------------------------------------------------ 7. retrieve (GPU)
def _corpus_module(T=64, Lq=9, N=6, Q=5, seed=601):
    from tests.test_shared_video import _module, _videos_and_queries
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=T, word_size=102)
    P = O.random_params(cfg, seed=seed)
    vb, qb = _videos_and_queries(cfg, N, Q, T, Lq, 6, seed=seed + 1)
    m = _module(cfg, P).to('cuda').eval()
    return cfg, P, {k: v.cuda() for k, v in vb.items()}, {k: v.cuda() for k, v in qb.items()}, m


def _host_retrieve(m, venc, qenc, lengths, k, nms_iou):
    """every query against every video in ONE localize_pairs call, the specification of extract_topk per pair, the specification of the merge"""
    from vslnet_amd.spans import topk_spans_reference
    Q, N = qenc.Q, venc.N
    q, v = np.repeat(np.arange(Q), N), np.tile(np.arange(N), Q)
    _, sl, el = m.localize_pairs(venc, qenc, v, q)
    s, e, sc, p, c = topk_spans_reference(sl.cpu().numpy(), el.cpu().numpy(), k, nms_iou, 0, lengths[v])
    return merge_topk_reference(s, e, sc, p.astype(np.float32), c, q, Q, k, v), p


@pytest.mark.gpu
def test_retrieve_equals_the_host_recomputation():
    cfg, P, dv, dq, m = _corpus_module()
    k = 5
    with torch.no_grad():
        venc = m.encode_video(dv['vfeats'], dv['v_mask'])
        qenc = m.encode_query(dq['word_ids'], dq['char_ids'], dq['q_mask'])
        got = m.retrieve(venc, qenc, k, nms_iou=0.5, pairs_per_call=12)            # 2 videos per chunk: three chunks and the second merge
        one = m.retrieve(venc, qenc, k, nms_iou=0.5)                               # one chunk
        lengths = dv['v_mask'].sum(dim=1).cpu().numpy().astype(np.int64)
        ref, allp = _host_retrieve(m, venc, qenc, lengths, k, 0.5)
    assert got.tag.shape == (5, k) and got.tag.dtype == torch.int32 and bool((got.count == k).all())
    # the test's own data: the reference keys that decide the first k + 1 ranks of a query are further apart than the `prob` gate allows the device's
    # to move, so the order is decidable
    for q in range(5):
        top = np.sort(allp[q * 6:(q + 1) * 6].reshape(-1))[::-1][:k + 1]
        assert np.all(top[:-1] - top[1:] > 2 * (1e-4 * top[:-1] + 1e-7)), (q, top)
    for nm, a, r in (('tag', got.tag, ref[0]), ('start', got.start, ref[2]), ('end', got.end, ref[3]), ('count', got.count, ref[6])):
        assert torch.equal(a.cpu(), torch.from_numpy(r)), (nm, a.cpu(), r)
    gp, rp = got.prob.cpu().double().numpy(), ref[5].astype(np.float64)
    err = np.abs(gp - rp) / (1e-4 * rp + 1e-7)
    print('retrieve: prob error %.3f of the gate' % float(err.max()))
    assert float(err.max()) <= 1.0
    for nm in ('tag', 'start', 'end', 'score', 'prob', 'count'):                   # chunked and unchunked: the same bits (`list` numbers other rows)
        assert torch.equal(getattr(got, nm), getattr(one, nm)), nm
    assert len(set(got.tag.cpu().reshape(-1).tolist())) > 1                        # the moments come from several videos


# ------------------------------------------------------------------------------------------------ 8. misuse (GPU)
@pytest.mark.gpu
def test_pairs_and_encode_query_refusals_by_name():
    import ctypes as C
    from tests.test_shared_video import _setup
    from vslnet_amd.engine import VslError, vsl_encode_query_io, vsl_io, vsl_pairs_io
    r = _row(3, 4, 96, 9)
    cfg, P, vb, qb, dv, dq, eng, flat, pg = _setup(r)
    vidx, qidx = [0, 2, 2, 1], [3, 0, 0, 2]
    # a saved-path forward, then the new calls in the same (shared) workspace: the backward and the taps are refused
    args = (flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dv['vfeats'][torch.tensor(vidx).cuda()].contiguous(),
            dv['v_mask'][torch.tensor(vidx).cuda()].contiguous(), dq['q_mask'])
    h, sl, el = eng.forward(*args, training=False)
    io = vsl_io()
    C.memmove(C.byref(io), C.byref(eng._last), C.sizeof(vsl_io))
    venc = eng.encode_video(flat, dv['vfeats'], dv['v_mask'])
    qenc = None
    for what in ('encode_query', 'localize_pairs'):
        if what == 'encode_query':
            qenc = eng.encode_query(flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dq['q_mask'])
        else:
            good = [t.clone() for t in eng.localize_pairs(flat, venc, qenc, vidx, qidx)]
        with pytest.raises(VslError, match='saved nothing'):
            eng.backward(torch.zeros_like(h), torch.zeros_like(sl), torch.zeros_like(el), eng.new_flat())
        with pytest.raises(VslError, match='saves nothing'):
            eng.ws_view('gated', (4, 96, 128))
        z, g = torch.zeros_like(sl), eng.new_flat()
        io.d_start_logits, io.d_end_logits, io.grads = z.data_ptr(), z.data_ptr(), g.data_ptr()
        assert eng.lib.vsl_backward(eng.h, C.byref(io), None) != 0 and b'the last forward saved nothing' in eng.lib.vsl_last_error(), what
        assert eng.lib.vsl_workspace_offset(eng.h, 4, 96, 9, 6, b'gated') == -2 and b'saved nothing' in eng.lib.vsl_last_error()
    # the raw entry point: every refusal by name
    idx32 = torch.tensor(vidx, dtype=torch.int32).cuda()
    qdx32 = torch.tensor(qidx, dtype=torch.int32).cuda()
    out = torch.empty(3, 4, 96, device='cuda')
    full = dict(B=4, T=96, Lq=9, N=3, Q=4, params=flat.data_ptr(), video_encoding=venc.encoding.data_ptr(), v_mask=venc.v_mask.data_ptr(),
                query_encoding=qenc.encoding.data_ptr(), q_mask=qenc.q_mask.data_ptr(), video_index=idx32.data_ptr(), query_index=qdx32.data_ptr(),
                h_score=out[0].data_ptr(), start_logits=out[1].data_ptr(), end_logits=out[2].data_ptr(), workspace=eng._ws.data_ptr())
    for change, text in ((dict(B=0), 'B=0'), (dict(N=0), 'N=0'), (dict(Q=0), 'Q=0'), (dict(Lq=129), 'Lq=129'), (dict(T=4097), 'T=4097'),
                         (dict(video_encoding=None), 'video_encoding is NULL'), (dict(query_encoding=None), 'query_encoding is NULL'),
                         (dict(v_mask=None), 'v_mask is NULL'), (dict(q_mask=None), 'q_mask is NULL'), (dict(video_index=None), 'video_index is NULL'),
                         (dict(query_index=None), 'query_index is NULL'), (dict(params=None), 'null device pointer'), (dict(workspace=None), 'null device pointer')):
        p_io = vsl_pairs_io(**dict(full, **change))
        assert eng.lib.vsl_localize_pairs(eng.h, C.byref(p_io), None) != 0 and text.encode() in eng.lib.vsl_last_error(), (change, eng.lib.vsl_last_error())
    p_io = vsl_pairs_io(**full)
    assert eng.lib.vsl_localize_pairs(eng.h, C.byref(p_io), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert all(torch.equal(a, c) for a, c in zip(good, out))
    e = vsl_encode_query_io()
    e.Q, e.Lq, e.Lc = 0, 9, 6
    assert eng.lib.vsl_encode_query(eng.h, C.byref(e), None) != 0 and b'Q=0' in eng.lib.vsl_last_error()
    e.Q = 4
    assert eng.lib.vsl_encode_query(eng.h, C.byref(e), None) != 0 and b'null device pointer' in eng.lib.vsl_last_error()
    n = C.c_int64()
    assert eng.lib.vsl_encode_query_workspace_floats(eng.h, 0, 9, 6, C.byref(n)) != 0 and b'Q=0' in eng.lib.vsl_last_error()
    assert eng.lib.vsl_encode_query_workspace_floats(eng.h, 4, 129, 6, C.byref(n)) != 0 and b'Lq=129' in eng.lib.vsl_last_error()
    # the binding: host indices are range-checked, handles type-checked
    with pytest.raises(ValueError, match='video_index out of range'):
        eng.localize_pairs(flat, venc, qenc, [0, 3, 2, 1], qidx)
    with pytest.raises(ValueError, match='query_index out of range'):
        eng.localize_pairs(flat, venc, qenc, vidx, [0, 4, 2, 1])
    with pytest.raises(ValueError, match='query_index'):
        eng.localize_pairs(flat, venc, qenc, vidx, qidx[:3])
    with pytest.raises(TypeError, match='QueryEncoding'):
        eng.localize_pairs(flat, venc, venc, vidx, qidx)
    with pytest.raises(ValueError, match='Q >= 1'):
        eng.encode_query(flat, pg[0], pg[1], dq['word_ids'][:0], dq['char_ids'][:0], dq['q_mask'][:0])
    eng.has_query_encoding = False                               # an older library: refused by name, no fallback
    try:
        with pytest.raises(VslError, match='no query encodings'):
            eng.encode_query(flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dq['q_mask'])
        with pytest.raises(VslError, match='no query encodings'):
            eng.localize_pairs(flat, venc, qenc, vidx, qidx)
    finally:
        eng.has_query_encoding = True
    assert all(torch.equal(a, c) for a, c in zip(good, eng.localize_pairs(flat, venc, qenc, vidx, qidx)))
    # the saved path again: backward and taps work
    eng.forward(*args, training=False)
    assert eng.ws_view('gated', (4, 96, 128)).shape == (4, 96, 128)


@pytest.mark.gpu
def test_module_handles_are_checked():
    from tests.test_shared_video import _module
    cfg, P, dv, dq, m = _corpus_module()
    q = (dq['word_ids'], dq['char_ids'], dq['q_mask'])
    vidx, qidx = [0, 5, 5, 2], [4, 0, 0, 1]
    with pytest.raises(RuntimeError, match='grad is enabled'):
        m.encode_query(*q)
    with torch.no_grad():
        venc, qenc = m.encode_video(dv['vfeats'], dv['v_mask']), m.encode_query(*q)
        out = [t.clone() for t in m.localize_pairs(venc, qenc, vidx, qidx)]
        ref = m.localize(venc, vidx, *(t[qidx] for t in q))
        assert all(torch.equal(a, c) for a, c in zip(out, ref)) and all(t.grad_fn is None for t in out)      # (8 heads, Lq 9: bit for bit)
    with pytest.raises(RuntimeError, match='grad is enabled'):
        m.localize_pairs(venc, qenc, vidx, qidx)
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match='train mode'):
        m.retrieve(venc, qenc, 3)
    m.eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match='stale VideoEncoding'):                  # train() may have changed the parameters
            m.localize_pairs(venc, qenc, vidx, qidx)
        venc = m.encode_video(dv['vfeats'], dv['v_mask'])
        with pytest.raises(ValueError, match='stale QueryEncoding'):
            m.localize_pairs(venc, qenc, vidx, qidx)
        with pytest.raises(ValueError, match='stale QueryEncoding'):
            m.retrieve(venc, qenc, 3)
        qenc = m.encode_query(*q)
        assert all(torch.equal(a, c) for a, c in zip(out, m.localize_pairs(venc, qenc, vidx, qidx)))
        other = _module(cfg, P).to('cuda').eval()
        with pytest.raises(ValueError, match='another module'):
            other.localize_pairs(venc, qenc, vidx, qidx)
        with pytest.raises(ValueError, match='another module'):
            m.localize_pairs(venc, other.encode_query(*q), vidx, qidx)
        m.load_state_dict(P, strict=True)
        with pytest.raises(ValueError, match='stale'):
            m.localize_pairs(venc, qenc, vidx, qidx)
        venc, qenc = m.encode_video(dv['vfeats'], dv['v_mask']), m.encode_query(*q)
        with pytest.raises(ValueError, match='pairs_per_call'):
            m.retrieve(venc, qenc, 3, pairs_per_call=4)


@pytest.mark.gpu
def test_a_training_step_before_and_after_the_new_calls_has_the_same_bits(monkeypatch):
    """One engine: a training step that meets the oracle; then encode_query, localize_pairs, extract_topk and merge_topk in its workspace; then the
    same step again.  It meets the oracle too and leaves the bits of the first: the saved activation `gated` and the whole gradient."""
    from tests.helpers import check_training_against_oracle
    from tests.test_shared_video import _videos_and_queries
    from vslnet_amd import engine as E
    B, T, Lq, Lc = 4, 96, 9, 6
    real, made = E.Engine, []

    def same_engine(cfg, *a, **k):
        if not made:
            made.append(real(cfg, *a, **k))
        return made[0]
    monkeypatch.setattr(E, 'Engine', same_engine)
    step = dict(cfg=dict(video_feature_dim=64), lazy=True)
    before = check_training_against_oracle(B, T, Lq, Lc, context='before the corpus calls', **step)
    eng, P = before.eng, before.P
    gated = eng.ws_view('gated', (B, T, 128)).clone()
    vb, qb = _videos_and_queries(O.make_cfg(video_feature_dim=64, max_pos_len=96, word_size=102, drop_rate=0.2), 3, 5, T, Lq, Lc, seed=702)
    pad, glove = P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda()
    venc = eng.encode_video(before.flat, vb['vfeats'].cuda(), vb['v_mask'].cuda())
    qenc = eng.encode_query(before.flat, pad, glove, qb['word_ids'].cuda(), qb['char_ids'].cuda(), qb['q_mask'].cuda())
    vidx, qidx = [0, 2, 2, 1, 0, 1], [4, 0, 0, 1, 3, 3]
    _, sl, el = eng.localize_pairs(before.flat, venc, qenc, vidx, qidx)
    spans = eng.extract_topk(sl, el, 4, nms_iou=0.5)
    m = eng.merge_topk(spans, torch.tensor(qidx, dtype=torch.int32).cuda(), 5, 4, tag=torch.tensor(vidx, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    assert int(m.count[0]) == 4 and int(m.count[2]) == 0                            # query 2 was asked about no video
    after = check_training_against_oracle(B, T, Lq, Lc, context='after the corpus calls', **step)
    assert len(made) == 1 and after.eng is eng
    assert torch.equal(eng.ws_view('gated', (B, T, 128)), gated) and torch.equal(after.g, before.g)


# ------------------------------------------------------------------------------------------------ 9. the evaluation loop and the CLI (GPU)
@pytest.mark.gpu
def test_eval_corpus_equals_a_host_recomputation():
    from model.VSLNet import VSLNet
    from tests.test_shared_video import _shared_dataset
    from vslnet_amd import runner
    from vslnet_amd.data import ResidentSplit
    from vslnet_amd.spans import TopK, topk_spans_reference
    from vslnet_amd.synthetic import make_configs
    configs = make_configs(video_feature_dim=64, max_pos_len=64, word_size=200, char_size=30, batch_size=6, drop_rate=0.2)
    recs, feats = _shared_dataset(configs, n_videos=5, per_video=3, seed=9)
    torch.manual_seed(5)
    m = VSLNet(configs, np.zeros((198, configs.word_dim), np.float32)).to('cuda').eval()
    split = ResidentSplit(recs, feats, configs, 'cuda', train=False)
    topk = TopK(3, 0.5, 0)
    stats, line = runner.eval_corpus(m, split, 'cuda', topk, pairs_per_call=12)      # 12 pairs: two videos per chunk at 6 queries, so both merge levels run
    assert set(stats) == {'k', 'corpus_r_k_i5', 'corpus_r_k_i7', 'video_recall_k'} and stats['k'] == 3
    assert line == 'Corpus Rank@3, IoU=0.5: %.2f\tIoU=0.7: %.2f\tvideo Recall@3: %.2f\n' % (stats['corpus_r_k_i5'], stats['corpus_r_k_i7'], stats['video_recall_k'])
    # the host: every batch's queries against every video through localize_pairs, the two specifications, the same hit rule
    best, found = [], []
    with torch.no_grad():
        venc = split.encode(m)
        lengths = venc.v_mask.sum(dim=1).cpu().numpy().astype(np.int64)
        for a in range(0, len(recs), 6):
            idx = np.arange(a, min(len(recs), a + 6))
            Lq, Lc = int(split.nwords[idx].max()), int(split.nchars[idx].max())
            words = split.d_words[idx[0]:idx[-1] + 1, :Lq].contiguous()
            chars = split.d_chars[idx[0]:idx[-1] + 1, :Lq, :Lc].contiguous()
            qenc = m.encode_query(words, chars, (words != 0).float())
            (tag, _, s, e, _, _, c), _ = _host_retrieve(m, venc, qenc, lengths, 3, 0.5)
            for q, i in enumerate(idx):
                b, f = runner.corpus_hits(tag[q], s[q], e[q], c[q], split.records[i], split.vid_of[i])
                best.append(b)
                found.append(f)
    want, _ = runner.summarise_corpus(best, found, 3)
    assert stats == want, (stats, want)
    assert 0.0 <= stats['corpus_r_k_i7'] <= stats['corpus_r_k_i5'] <= stats['video_recall_k'] <= 100.0
    with pytest.raises(ValueError, match='needs topk'):
        runner.eval_corpus(m, split, 'cuda', None)


def test_corpus_arithmetic_and_cli_flag():
    import main as cli
    from vslnet_amd import runner
    rec = dict(s_time=2.0, e_time=6.0, v_len=10, duration=10.0)
    # clip i covers [i, i + 1) s: (2, 5) is the ground truth -- but only in video 3
    assert runner.corpus_hits([1, 3, 3], [2, 0, 2], [5, 0, 5], 3, rec, 3) == (1.0, True)
    assert runner.corpus_hits([1, 2, 3], [2, 2, 2], [5, 5, 5], 2, rec, 3) == (0.0, False)        # the slot in video 3 is beyond count
    assert runner.corpus_hits([3, -1, -1], [0, -1, -1], [0, -1, -1], 1, rec, 3) == (0.0, True)   # the right video, the wrong moment
    stats, line = runner.summarise_corpus([1.0, 0.0, 0.6, 0.0], [True, False, True, True], 5)
    assert stats == {'k': 5, 'corpus_r_k_i5': 50.0, 'corpus_r_k_i7': 25.0, 'video_recall_k': 75.0}
    assert line == 'Corpus Rank@5, IoU=0.5: 50.00\tIoU=0.7: 25.00\tvideo Recall@5: 75.00\n'
    ns = cli.build_parser().parse_args([])
    assert ns.corpus is False and cli.check_corpus(ns) is False
    assert cli.check_corpus(cli.build_parser().parse_args(['--corpus', '--topk', '5'])) is False            # (--mode train only stores the flag)
    assert cli.check_corpus(cli.build_parser().parse_args(['--mode', 'test', '--corpus', '--topk', '5'])) is True
    with pytest.raises(ValueError, match='--topk K >= 1'):
        cli.check_corpus(cli.build_parser().parse_args(['--mode', 'test', '--corpus']))
    with pytest.raises(ValueError, match='--data resident'):
        cli.check_corpus(cli.build_parser().parse_args(['--mode', 'test', '--corpus', '--topk', '5', '--data', 'loader']))


@pytest.mark.gpu
def test_cli_reports_corpus_numbers_only_when_asked(tmp_path):
    import json
    import main as cli
    argv = ['--task', 'synthetic', '--predictor', 'transformer', '--max_pos_len', '32', '--video_feature_dim', '64', '--batch_size', '16', '--epochs', '1',
            '--period', '100', '--synthetic_train', '64', '--synthetic_test', '32', '--model_dir', str(tmp_path), '--topk', '3']
    out = cli.run(argv + ['--mode', 'train'], log=lambda *a: None)
    assert json.load(open(os.path.join(out['model_dir'], 'configs.json')))['corpus'] is False      # stored like the other flags
    plain, asked = [], []
    res = cli.run(argv + ['--mode', 'test'], log=plain.append)
    res_c = cli.run(argv + ['--mode', 'test', '--corpus'], log=asked.append)
    # without the flag: the eight lines of Rank@1 + Rank@3 and their keys, nothing of the corpus
    assert len(plain) == 8 and not [x for x in plain if 'orpus' in x or 'Recall' in x] and not [k for k in res if 'corpus' in k or 'recall' in k]
    # with it: the same bytes first, then three more lines
    assert asked[:8] == plain and len(asked) == 11 and {k: v for k, v in res_c.items() if k in res} == res
    assert asked[8].startswith('\x1b[1;31mCorpus Rank@3, IoU=0.5:\t') and asked[10].startswith('\x1b[1;31mvideo Recall@3:\t')
    assert 0.0 <= res_c['corpus_r_k_i7'] <= res_c['corpus_r_k_i5'] <= res_c['video_recall_k'] <= 100.0
