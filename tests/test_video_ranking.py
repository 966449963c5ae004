"""Two-stage corpus search on the device: vsl_highlight_pairs + k_pair_relevance, vsl_select_topm, Engine.highlight_pairs / select_topm,
VSLNet.rank_videos and VSLNet.retrieve(prefilter=M).

The specifications are vslnet_amd.spans.pair_relevance_reference / select_topm_reference (checked on the CPU in tests/test_video_ranking_spec.py) and, for
the second stage, merge_topk_reference.  Everything but the mean relevance is compared for EQUALITY: the select is a strict total order, the max is
exact, h_score comes from the kernels of localize_pairs in their order, and retrieve(prefilter >= N) is the exhaustive search.  The mean is gated at
1e-6 relative against the fp64 specification: at most 64 positive fp32 terms summed in 6 + 1 levels of a tree, each within 2^-24 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from vslnet_amd.spans import merge_topk_reference, pair_relevance_reference, select_topm_reference

pytestmark = pytest.mark.gpu

Q, N_VIDEOS, LQ, LC, DV = 3, 7, 6, 5, 64


# ------------------------------------------------------------------------------------------------ 1. select_topm against the specification
_ENGINE = {}


def _engine():
    """one small engine for the free-standing select calls (they read no plan and no parameters)"""
    if 'eng' not in _ENGINE:
        from vslnet_amd.engine import Engine
        _ENGINE['eng'] = Engine(O.make_cfg(video_feature_dim=DV, max_pos_len=32, word_size=102))
    return _ENGINE['eng']


def _boundary_ties(G, N, take, rng):
    """zeros, `take // 2` keys of 2.0 somewhere, and a run of 1.0 around index 256 (the middle of a shorter row) longer than the ties still to take:
    the threshold key 1.0 is shared by indices on both sides of a 256-element boundary, and only the first of them may be selected"""
    key = np.zeros((G, N), np.float32)
    ties = take - take // 2
    mid = 256 if N > 258 else N // 2
    lo, hi = max(0, mid - (ties + 1) // 2 - 1), min(N, mid + ties // 2 + 3)
    for g in range(G):
        key[g, lo:hi] = 1.0
        rest = np.setdiff1d(np.arange(N), np.arange(lo, hi))
        key[g, rng.permutation(rest)[:take // 2]] = 2.0
    return key


def _keys(kind, G, N, take, rng):
    if kind == 'equal':
        return np.full((G, N), 0.75, np.float32)
    if kind == 'four':
        return np.array([-1.0, 0.25, 0.5, 3.0], np.float32)[rng.integers(0, 4, size=(G, N))]
    if kind == 'random':
        return rng.standard_normal((G, N)).astype(np.float32)
    if kind == 'special':                                    # -inf, +0.0 and -0.0 (and a few ordinary keys) in every row
        return np.array([-np.inf, 0.0, -0.0, 0.0, -0.0, 1.0, -1.0], np.float32)[rng.integers(0, 7, size=(G, N))]
    return _boundary_ties(G, N, take, rng)


def test_boundary_rows_put_the_threshold_on_both_sides_of_256():
    """(the generator does what the case is about -- checked once, on the host)"""
    key = _boundary_ties(1, 1000, 64, np.random.default_rng(0))
    index, out_key, _ = select_topm_reference(key, 64)
    taken = index[0][out_key[0] == 1.0]
    assert taken.min() < 256 <= taken.max() and (key[0] == 1.0).sum() > len(taken) and np.flatnonzero(key[0] == 1.0).max() > taken.max()


@pytest.mark.parametrize('kind', ['equal', 'four', 'random', 'special', 'boundary'])
def test_select_topm_equals_the_specification(kind):
    eng = _engine()
    rng = np.random.default_rng(['equal', 'four', 'random', 'special', 'boundary'].index(kind))
    cases = 0
    for N in (1, 5, 255, 256, 257, 1000, 1025, 5000):
        for M in sorted({1, 3, N - 1, N, N + 7, 1024}):
            if not 1 <= M <= 1024:                           # (refused: test_refusals_by_name)
                continue
            for G in (1, 3):
                key = _keys(kind, G, N, min(M, N), rng)
                want = select_topm_reference(key, M)
                for pad in (0, 3):                           # ld = N and ld = N + 3: a column slice of a wider matrix
                    wide = torch.full((G, N + pad), float('nan'), device='cuda')
                    wide[:, :N] = torch.from_numpy(key).cuda()
                    got = eng.select_topm(wide[:, :N], M)
                    again = eng.select_topm(wide[:, :N], M)
                    assert got.video.dtype == torch.int32 and got.video.shape == (G, M) and got.count.dtype == torch.int32
                    for nm, a, b, w in zip(('index', 'key', 'count'), got, again, want):
                        assert torch.equal(a, b), (kind, N, M, G, pad, nm, 'two runs differ')
                        assert np.array_equal(a.cpu().numpy(), w), (kind, N, M, G, pad, nm, a.cpu().numpy(), w)
                    z = got.relevance.cpu().numpy()
                    assert not np.signbit(z[z == 0]).any()   # -0.0 is returned as +0.0
                    cases += 1
    assert cases >= 100


# ------------------------------------------------------------------------------------------------ 2. highlight_pairs
def _row(T, predictor='transformer'):
    return dict(N=N_VIDEOS, B=Q, idx=None, T=T, Lq=LQ, heads=8, predictor=predictor, Dv=DV, ragged=True, extreme=False, bf16=False, word_table=False, Lc=LC)


HIGHLIGHT_CASES = [pytest.param(32, 'transformer', id='T32'), pytest.param(64, 'transformer', id='T64'), pytest.param(45, 'transformer', id='T45'),
                   pytest.param(45, 'rnn', id='T45-rnn')]


@pytest.mark.parametrize('T,predictor', HIGHLIGHT_CASES)
def test_highlight_pairs_equals_localize_pairs_and_the_specification(T, predictor):
    from tests.test_shared_video import _ledger, _setup
    from vslnet_amd.engine import VideoEncoding
    cfg, P, vb, qb, dv, dq, eng, flat, pg = _setup(_row(T, predictor))
    assert eng.has_video_ranking
    lens = dv['v_mask'].sum(dim=1).long().cpu().numpy()
    assert len(set(lens.tolist())) > 2 and lens.max() == T                   # videos of different valid lengths
    venc = eng.encode_video(flat, dv['vfeats'], dv['v_mask'])
    mask = dv['v_mask'].clone()
    mask[4] = 0                                                               # a video of valid length 0: same encoding, an all-pad mask
    venc = VideoEncoding(venc.encoding, mask)
    qenc = eng.encode_query(flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dq['q_mask'])
    qi, vi = np.repeat(np.arange(Q), N_VIDEOS), np.tile(np.arange(N_VIDEOS), Q)
    h_ref, names_loc = _ledger(eng, lambda: eng.localize_pairs(flat, venc, qenc, vi, qi)[0].clone())
    pair_mask = mask[torch.from_numpy(vi).cuda()].cpu().numpy()
    for mode in ('max', 'mean'):
        h = torch.full((Q * N_VIDEOS, T), float('nan'), device='cuda')
        (vec, names) = _ledger(eng, lambda: eng.highlight_pairs(flat, venc, qenc, vi, qi, relevance=mode, h_score=h).clone())
        assert torch.equal(h, h_ref), (mode, float((h - h_ref).abs().max()))
        # the launches: those of localize_pairs up to cq_out, in its order, then the reduction; no predictor, no heads
        assert names[-2:] == ['cq_out', 'pair_relevance'] and names[:-1] == names_loc[:len(names) - 1] and len(names_loc) > len(names), (names, names_loc)
        assert set(names) <= {'vmask_gather', 'pack', 'cq_score', 'cq_col', 'cq_out', 'pair_relevance'}, names
        want = pair_relevance_reference(h_ref.cpu().numpy(), pair_mask, mode)
        got = vec.cpu().numpy()
        assert np.isneginf(got[vi == 4]).all() and np.isneginf(want[vi == 4]).all() and np.isfinite(got[vi != 4]).all()
        if mode == 'max':
            assert np.array_equal(got, want), (got, want)
        else:
            live = vi != 4
            err = np.abs(got[live].astype(np.float64) - want[live]) / np.abs(want[live])
            print('mean relevance: max relative error %.3g' % float(err.max()))
            assert float(err.max()) <= 1e-6
        # the (Q, ld) matrix write agrees with the vector write and touches nothing else; without the h_score buffer: the same values
        ld = N_VIDEOS + 2
        matrix = torch.full((Q, ld), float('nan'), device='cuda')
        assert eng.highlight_pairs(flat, venc, qenc, vi, qi, relevance=mode, out=matrix, ld=ld) is matrix
        assert torch.equal(matrix[:, :N_VIDEOS].reshape(-1), vec) and bool(torch.isnan(matrix[:, N_VIDEOS:]).all())
        # the same pairs in another order land in the same cells with the same bits (whole tiles: the pair kernels do not depend on the position)
        if T % 32 == 0:
            perm = np.random.default_rng(T).permutation(Q * N_VIDEOS)
            m2 = torch.full((Q, N_VIDEOS), float('nan'), device='cuda')
            eng.highlight_pairs(flat, venc, qenc, vi[perm], qi[perm], relevance=mode, out=m2, ld=N_VIDEOS)
            assert torch.equal(m2.reshape(-1), vec)
    # the workspace is marked like an inference forward
    from vslnet_amd.engine import VslError
    with pytest.raises(VslError, match='saves nothing'):
        eng.ws_view('gated', (Q * N_VIDEOS, T, 128))


# ------------------------------------------------------------------------------------------------ 3. rank_videos and retrieve
_MODULES = {}


def _corpus(T):
    """one module, N videos and Q queries per T, encoded once and shared by the tests below (nothing here is modified afterwards)"""
    if T not in _MODULES:
        from tests.test_shared_video import _module, _videos_and_queries
        cfg = O.make_cfg(video_feature_dim=DV, max_pos_len=T, word_size=102)
        P = O.random_params(cfg, seed=701)
        vb, qb = _videos_and_queries(cfg, N_VIDEOS, Q, T, LQ, LC, seed=702 + T)
        m = _module(cfg, P).to('cuda').eval()
        with torch.no_grad():
            venc = m.encode_video(vb['vfeats'].cuda(), vb['v_mask'].cuda())
            qenc = m.encode_query(qb['word_ids'].cuda(), qb['char_ids'].cuda(), qb['q_mask'].cuda())
        _MODULES[T] = (m, venc, qenc)
    return _MODULES[T]


@pytest.mark.parametrize('T', [32, 64])
@pytest.mark.parametrize('relevance', ['max', 'mean'])
def test_rank_videos_equals_the_select_of_the_librarys_own_matrix(T, relevance):
    m, venc, qenc = _corpus(T)
    qi, vi = np.repeat(np.arange(Q), N_VIDEOS), np.tile(np.arange(N_VIDEOS), Q)
    matrix = torch.empty(Q, N_VIDEOS, device='cuda')
    with torch.no_grad():
        m._engine.highlight_pairs(m._flat, venc, qenc, vi, qi, relevance=relevance, out=matrix, ld=N_VIDEOS)
        for mm in (1, 2, N_VIDEOS, N_VIDEOS + 3):
            want = select_topm_reference(matrix.cpu().numpy(), mm)
            one = m.rank_videos(venc, qenc, mm, relevance=relevance)
            chunked = m.rank_videos(venc, qenc, mm, relevance=relevance, pairs_per_call=6)       # two videos per chunk: four chunks
            for nm, a, b, w in zip(('video', 'relevance', 'count'), one, chunked, want):
                assert np.array_equal(a.cpu().numpy(), w), (mm, nm, a, w)
                assert torch.equal(a, b), (mm, nm, 'the chunking shows')
    assert len({tuple(r) for r in one.video.cpu().tolist()}) > 1 or Q == 1                      # (the queries do not all rank the videos alike)


FIELDS = ('tag', 'list', 'start', 'end', 'score', 'prob', 'count')


@pytest.mark.parametrize('T', [32, 64])
def test_retrieve_with_every_video_kept_is_the_exhaustive_search(T):
    m, venc, qenc = _corpus(T)
    with torch.no_grad():
        for per_call in (4096, 6):                                            # one chunk ; two videos / six pairs per chunk and the second merge
            want = m.retrieve(venc, qenc, 3, nms_iou=0.5, pairs_per_call=per_call)
            for keep in (N_VIDEOS, N_VIDEOS + 5, 5000):                       # (above 1024 with N <= 1024: "all videos")
                got = m.retrieve(venc, qenc, 3, nms_iou=0.5, pairs_per_call=per_call, prefilter=keep)
                for nm in FIELDS:
                    assert torch.equal(getattr(got, nm), getattr(want, nm)), (T, per_call, keep, nm, getattr(got, nm), getattr(want, nm))
            got, ranks = m.retrieve(venc, qenc, 3, nms_iou=0.5, pairs_per_call=per_call, prefilter=N_VIDEOS, relevance='mean', return_ranks=True)
            assert all(torch.equal(getattr(got, nm), getattr(want, nm)) for nm in FIELDS) and ranks.video.shape == (Q, N_VIDEOS)
    assert bool((want.count == 3).all()) and len(set(want.tag.cpu().reshape(-1).tolist())) > 1


@pytest.mark.parametrize('T', [32, 64])
def test_retrieve_with_a_prefilter_is_the_exhaustive_search_restricted_to_the_selected_pairs(T):
    m, venc, qenc = _corpus(T)
    k, keep = 3, 2
    qi, vi = np.repeat(np.arange(Q), N_VIDEOS), np.tile(np.arange(N_VIDEOS), Q)
    with torch.no_grad():
        # the exhaustive per-pair lists: one localize_pairs call over all pairs, the library's extract_topk
        _, sl, el = m.localize_pairs(venc, qenc, vi, qi)
        lengths = venc.v_mask.sum(dim=1).to(torch.int32)
        spans = m.extract_topk(sl, el, k, nms_iou=0.5, lengths=lengths[torch.from_numpy(vi).cuda()], want_prob=True)
        ranks = m.rank_videos(venc, qenc, keep)
        selected = np.zeros((Q, N_VIDEOS), bool)
        np.put_along_axis(selected, ranks.video.cpu().numpy().astype(np.int64), True, axis=1)
        count = np.where(selected.reshape(-1), spans.count.cpu().numpy(), 0)                    # a pair that was not selected offers no candidate
        want = merge_topk_reference(spans.start.cpu().numpy(), spans.end.cpu().numpy(), spans.score.cpu().numpy(), spans.prob.cpu().numpy(), count, qi, Q, k, vi)
        for per_call in (4096, 3, 4):                                         # one chunk ; chunks of one query's pairs and a half ; chunks that split a query
            got, r2 = m.retrieve(venc, qenc, k, nms_iou=0.5, pairs_per_call=per_call, prefilter=keep, return_ranks=True)
            assert all(torch.equal(a, b) for a, b in zip(r2, ranks))
            for nm, w in zip(FIELDS, want):
                if nm == 'list' and per_call != 4096:                         # (chunked: `list` numbers the rows of the exhaustive search's second merge)
                    continue
                assert np.array_equal(getattr(got, nm).cpu().numpy(), w), (T, per_call, nm, getattr(got, nm), w)
    tags = got.tag.cpu().numpy()
    assert all(set(tags[q][tags[q] >= 0]) <= set(np.flatnonzero(selected[q])) for q in range(Q))


# ------------------------------------------------------------------------------------------------ 4. refusals, each by name
def test_refusals_by_name():
    from vslnet_amd.engine import VideoEncoding, VslError, vsl_highlight_io
    m, venc, qenc = _corpus(32)
    eng = m._engine
    key = torch.zeros(2, 9, device='cuda')
    for M, text in ((0, r'M=0 must be in \[1, 1024\]'), (1025, r'M=1025 must be in \[1, 1024\]'), (-3, 'M=-3')):
        with pytest.raises(VslError, match=text):
            eng.select_topm(key, M)
    with pytest.raises(VslError, match='ld=4 must be at least N=9'):
        eng.select_topm(torch.as_strided(torch.zeros(16, device='cuda'), (2, 9), (4, 1)), 3)
    with pytest.raises(ValueError, match='contiguous rows'):
        eng.select_topm(key.t(), 3)
    vi, qi = [0, 1, 2], [0, 0, 1]
    with pytest.raises(ValueError, match="relevance must be 'max' or 'mean'"):
        eng.highlight_pairs(m._flat, venc, qenc, vi, qi, relevance='sum')
    with pytest.raises(ValueError, match='video_index out of range'):
        eng.highlight_pairs(m._flat, venc, qenc, [0, N_VIDEOS, 2], qi)
    with pytest.raises(ValueError, match='pass it as out'):
        eng.highlight_pairs(m._flat, venc, qenc, vi, qi, ld=N_VIDEOS)
    # the raw entry point
    good = eng.highlight_pairs(m._flat, venc, qenc, vi, qi).clone()
    vidx, qidx = torch.tensor(vi, dtype=torch.int32).cuda(), torch.tensor(qi, dtype=torch.int32).cuda()
    out = torch.empty(Q * N_VIDEOS, device='cuda')
    pairs = dict(B=3, T=32, Lq=LQ, N=N_VIDEOS, Q=Q, params=m._flat.data_ptr(), video_encoding=venc.encoding.data_ptr(), v_mask=venc.v_mask.data_ptr(),
                 query_encoding=qenc.encoding.data_ptr(), q_mask=qenc.q_mask.data_ptr(), video_index=vidx.data_ptr(), query_index=qidx.data_ptr(),
                 workspace=eng._ws.data_ptr())
    top = dict(relevance=0, ld=0, out=out.data_ptr())

    def call(pairs_change=(), **top_change):
        io = vsl_highlight_io()
        for k2, v in dict(pairs, **dict(pairs_change)).items():
            setattr(io.pairs, k2, v)
        for k2, v in dict(top, **top_change).items():
            setattr(io, k2, v)
        rc = eng.lib.vsl_highlight_pairs(eng.h, C.byref(io), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, eng.lib.vsl_last_error()

    for change, text in ((dict(B=0), 'B=0'), (dict(N=0), 'N=0'), (dict(Q=0), 'Q=0'), (dict(Lq=129), 'Lq=129'), (dict(T=4097), 'T=4097'),
                         (dict(video_encoding=None), 'video_encoding is NULL'), (dict(query_encoding=None), 'query_encoding is NULL'),
                         (dict(v_mask=None), 'v_mask is NULL'), (dict(q_mask=None), 'q_mask is NULL'), (dict(video_index=None), 'video_index is NULL'),
                         (dict(query_index=None), 'query_index is NULL'), (dict(params=None), 'null device pointer'), (dict(workspace=None), 'null device pointer')):
        rc, err = call(change)
        assert rc != 0 and b'vsl_highlight' in err and text.encode() in err, (change, err)
    for change, text in ((dict(relevance=2), 'relevance=2 must be 0 (max) or 1 (mean)'), (dict(relevance=-1), 'relevance=-1'), (dict(out=None), 'out is NULL'),
                         (dict(ld=N_VIDEOS - 1), 'ld=%d must be 0' % (N_VIDEOS - 1)), (dict(ld=1), 'ld=1 must be 0'), (dict(ld=-1), 'ld=-1')):
        rc, err = call(**change)
        assert rc != 0 and text.encode() in err, (change, err)
    rc, err = call()                                                          # the logits pointers and h_score are not needed
    assert rc == 0, err
    assert torch.equal(out[:3], good)
    # the module: modes, handles, limits
    with pytest.raises(RuntimeError, match='grad is enabled'):
        m.rank_videos(venc, qenc, 2)
    with torch.no_grad():
        with pytest.raises(ValueError, match='pairs_per_call=2 is less than one video'):
            m.rank_videos(venc, qenc, 2, pairs_per_call=2)
        with pytest.raises(ValueError, match='prefilter=-1'):
            m.retrieve(venc, qenc, 3, prefilter=-1)
        with pytest.raises(VslError, match=r'M=1025 must be in \[1, 1024\]'):
            m.rank_videos(venc, qenc, 1025)
        # more than 1024 videos: the argument check alone, on a handle that owns no real corpus
        big = VideoEncoding(torch.empty(1025, 1, 128, device='cuda'), torch.ones(1025, 1, device='cuda'), owner=m, epoch=m._param_epoch)
        with pytest.raises(ValueError, match='prefilter=1025 with N=1025 videos: the first stage selects at most 1024'):
            m.retrieve(big, qenc, 3, prefilter=1025)
        # a library without the entry points: the first stage is refused by name, the exhaustive search is served
        want = m.retrieve(venc, qenc, 3)
        eng.has_video_ranking = False
        try:
            with pytest.raises(VslError, match='vsl_highlight_pairs / vsl_select_topm are missing'):
                m.retrieve(venc, qenc, 3, prefilter=2)
            with pytest.raises(VslError, match='cannot rank videos'):
                m.rank_videos(venc, qenc, 2)
            again = m.retrieve(venc, qenc, 3)
        finally:
            eng.has_video_ranking = True
        assert all(torch.equal(a, b) for a, b in zip(want, again))
        # a stale handle (LAST: the shared encodings of this T are stale from here on)
        m.train()
        m.eval()
        with pytest.raises(ValueError, match='stale VideoEncoding'):
            m.retrieve(venc, qenc, 3, prefilter=2)
        with pytest.raises(ValueError, match='stale VideoEncoding'):
            m.rank_videos(venc, qenc, 2)
    del _MODULES[32]
