"""Top-K moments per query (vsl_extract_topk): the numpy specification on the CPU (the worked example, agreement with the oracle's extract_index,
the properties of greedy NMS, the Rank@K arithmetic, the CLI flags), and the kernel against that specification on the GPU: start / end / count / score
bit for bit, `prob` within 1e-4 * ref + 1e-7, ties, exhaustion, T = 4096, misuse, determinism, independence of the handle's state, the eval loops."""
import functools

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from vslnet_amd import runner
from vslnet_amd.spans import TopK, spans_to_times, suppressed, topk_spans_reference

MASK_VALUE = -1e30


def _pairs(out, b=0):
    s, e, sc, _, c = out
    return [(int(s[b, r]), int(e[b, r]), float(sc[b, r])) for r in range(int(c[b]))]


# ------------------------------------------------------------------------------------------------ CPU: the specification
def test_worked_example():
    sl, el = np.array([[0, 1, 0]], dtype=np.float32), np.array([[0, 0, 1]], dtype=np.float32)
    assert _pairs(topk_spans_reference(sl, el, 32, 1.0)) == [(1, 2, 2.0), (0, 2, 1.0), (1, 1, 1.0), (2, 2, 1.0), (0, 0, 0.0), (0, 1, 0.0)]
    assert _pairs(topk_spans_reference(sl, el, 32, 0.5)) == [(1, 2, 2.0), (1, 1, 1.0), (2, 2, 1.0), (0, 0, 0.0), (0, 1, 0.0)]      # (0, 2): inter 2 > 0.5 * 3
    assert _pairs(topk_spans_reference(sl, el, 32, 0.0)) == [(1, 2, 2.0), (0, 0, 0.0)]
    out = topk_spans_reference(sl, el, 32, 1.0, max_span=1, lengths=[2])
    assert _pairs(out) == [(1, 1, 1.0), (0, 0, 0.0)]
    s, e, sc, p, c = out
    assert c[0] == 2 and (s[0, 2:] == -1).all() and (e[0, 2:] == -1).all() and np.isneginf(sc[0, 2:]).all() and (p[0, 2:] == 0).all()
    assert sc.dtype == np.float32 and s.dtype == np.int64 and c.dtype == np.int32


def _seeded_case(seed):
    """the 200 seeded cases: T uniform in 1 .. 299, logits 3 N(0, 1) float32"""
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, 300))
    return (3.0 * rng.standard_normal((1, T))).astype(np.float32), (3.0 * rng.standard_normal((1, T))).astype(np.float32)


def test_top1_without_nms_is_the_oracles_extract_index():
    bad = 0
    for seed in range(200):
        sl, el = _seeded_case(seed)
        s, e, _, _, c = topk_spans_reference(sl, el, 1, 1.0, 0)
        osi, oei = O.extract_index(torch.from_numpy(sl), torch.from_numpy(el))
        bad += not (c[0] == 1 and int(s[0, 0]) == int(osi[0]) and int(e[0, 0]) == int(oei[0]))
    assert bad == 0


def test_properties_of_the_greedy_selection():
    rng = np.random.default_rng(77)
    for case in range(40):
        T, K = int(rng.integers(1, 40)), int(rng.choice([1, 5, 32]))
        nms, max_span = float(rng.choice([1.0, 0.5, 0.3, 0.0])), int(rng.choice([0, 1, 4]))
        L = int(rng.integers(1, T + 1))
        sl, el = (rng.integers(-3, 4, (1, T)).astype(np.float32) if case % 2 else (3 * rng.standard_normal((1, T))).astype(np.float32) for _ in range(2))
        s, e, sc, p, c = topk_spans_reference(sl, el, K, nms, max_span, lengths=[L])
        n = int(c[0])
        spans = [(int(s[0, r]), int(e[0, r])) for r in range(n)]
        assert all(sc[0, r] >= sc[0, r + 1] for r in range(n - 1))                         # scores are non-increasing
        assert len(set(spans)) == n
        for q, (a0, a1) in enumerate(spans):
            assert 0 <= a0 <= a1 < L and (max_span == 0 or a1 - a0 + 1 <= max_span)
            assert sc[0, q] == np.float32(sl[0, a0]) + np.float32(el[0, a1])
            assert not any(suppressed(a0, a1, b0, b1, nms) for b0, b1 in spans[:q])         # no later span is suppressed by an earlier one
        ncand = sum(1 for i in range(L) for j in range(i, L) if max_span == 0 or j - i + 1 <= max_span)
        if nms == 1.0:
            assert n == min(K, ncand)
        assert n >= 1 and n <= min(K, ncand) and (p[0, :n] > 0).all() and (p[0, n:] == 0).all()


def test_rank_at_k_arithmetic():
    rec = [dict(s_time=2.0, e_time=6.0, v_len=10, duration=10.0), dict(s_time=0.0, e_time=1.0, v_len=10, duration=10.0),
           dict(s_time=5.0, e_time=9.0, v_len=10, duration=10.0)]
    # clip i covers [i, i + 1) s here: span (s, e) is [s, e + 1] seconds
    spans = [([0, 2, 7], [0, 5, 8], 3), ([4, 0, -1], [9, 0, -1], 2), ([0, 1, 2], [0, 1, 2], 0)]
    assert spans_to_times(np.array([2, 7]), np.array([5, 8]), 2, 10, 10.0) == [(2.0, 6.0), (7.0, 9.0)]
    best = [runner.best_iou_of_spans(np.array(s), np.array(e), c, r) for (s, e, c), r in zip(spans, rec)]
    first = [runner.calculate_iou(list(spans_to_times(np.array(s), np.array(e), 1, r['v_len'], r['duration'])[0]), [r['s_time'], r['e_time']])
             for (s, e, c), r in zip(spans, rec)]
    assert best[0] == 1.0 and first[0] == 0.0                    # the second span is the ground truth, the first misses it
    assert best[1] == 1.0 and first[1] == 0.0                    # (the fill slot beyond count is not read)
    assert best[2] == 0.0                                        # count 0: no span, IoU 0
    stats, line = runner.summarise_topk(best, 3)
    assert stats == {'k': 3, 'r_k_i3': pytest.approx(200.0 / 3.0), 'r_k_i5': pytest.approx(200.0 / 3.0), 'r_k_i7': pytest.approx(200.0 / 3.0),
                     'mIoU_k': pytest.approx(200.0 / 3.0)}
    assert line == 'Rank@3, IoU=0.3: 66.67\tIoU=0.5: 66.67\tIoU=0.7: 66.67\tbest-of-3 mean IoU: 66.67\n'
    r1 = runner.summarise(first)
    assert all(stats[k] >= v for k, v in zip(('r_k_i3', 'r_k_i5', 'r_k_i7', 'mIoU_k'), r1[:4]))      # R@K >= R@1


def test_cli_flags_default_to_off():
    import main as cli
    ns = cli.build_parser().parse_args([])
    assert (ns.topk, ns.nms_iou, ns.max_span) == (0, 0.5, 0) and cli.topk_of(ns) is None
    ns = cli.build_parser().parse_args(['--topk', '5', '--nms_iou', '0.3', '--max_span', '12'])
    assert cli.topk_of(ns) == TopK(5, 0.3, 12)
    for bad in (['--topk', '33'], ['--topk', '5', '--nms_iou', '1.5'], ['--topk', '5', '--max_span', '-1']):
        with pytest.raises(ValueError):
            cli.topk_of(cli.build_parser().parse_args(bad))


# ------------------------------------------------------------------------------------------------ GPU: the kernel against the specification
@functools.lru_cache(maxsize=None)
def _engine():
    from vslnet_amd.engine import Engine
    return Engine(O.make_cfg(video_feature_dim=64, max_pos_len=32, word_size=52))


def _lengths(rng, kind, B, T):
    if kind == 'none':
        return None
    L = rng.integers(1, T + 1, B)
    if kind == 'edge':                                           # 1 and T among them
        L[0] = T
        L[B - 1] = 1 if B > 1 else T
        if B > 2:
            L[1] = 1
            L[B - 1] = T
    return L.astype(np.int64)


def _logits(rng, B, T, lengths, integers=False, clip=True):
    """3 N(0, 1) (clip: cut to |x| <= 8, the range the `prob` gate is derived for; or integers -2 .. 2), MASK_VALUE added beyond the length, as the
    model emits them"""
    out = []
    for _ in range(2):
        x = rng.integers(-2, 3, (B, T)).astype(np.float32) if integers else (3.0 * rng.standard_normal((B, T))).astype(np.float32)
        if clip:
            x = np.clip(x, -8.0, 8.0)
        if lengths is not None:
            x = x + (np.arange(T)[None, :] >= np.asarray(lengths)[:, None]).astype(np.float32) * np.float32(MASK_VALUE)
        out.append(np.ascontiguousarray(x, dtype=np.float32))
    return out


#        B    T    K  nms  span lengths
CASES = [(1, 1, 1, 1.0, 0, 'none'), (3, 2, 5, 0.5, 0, 'none'), (3, 3, 32, 0.0, 1, 'edge'), (64, 31, 5, 0.5, 7, 'ragged'), (3, 32, 32, 0.5, 0, 'ragged'),
         (64, 33, 1, 1.0, 0, 'ragged'), (3, 117, 32, 0.5, 7, 'edge'), (3, 117, 5, 0.0, 0, 'none'), (1, 255, 32, 0.5, 0, 'none'),
         (3, 256, 5, 1.0, 7, 'ragged'), (3, 256, 32, 0.0, 0, 'edge'), (3, 257, 32, 0.5, 0, 'ragged'), (1, 257, 5, 1.0, 1, 'none'),
         (3, 511, 5, 0.5, 0, 'edge'), (1, 511, 32, 0.0, 7, 'ragged'), (3, 1024, 5, 0.5, 0, 'ragged'), (1, 1024, 1, 1.0, 0, 'none'),
         (3, 1024, 5, 0.0, 7, 'edge'), (64, 32, 32, 1.0, 0, 'none'), (3, 33, 5, 0.5, 1, 'edge')]


def _run(sl, el, K, nms, span, lengths, **kw):
    return _engine().extract_topk(torch.from_numpy(sl).cuda(), torch.from_numpy(el).cuda(), K, nms_iou=nms, max_span=span,
                                  lengths=None if lengths is None else torch.from_numpy(lengths).cuda(), **kw)


def _assert_exact(got, ref, context, gate_prob=True):
    s, e, sc, p, c = ref
    assert got.start.dtype == torch.int64 and got.end.dtype == torch.int64 and got.score.dtype == torch.float32 and got.count.dtype == torch.int32
    assert torch.equal(got.count.cpu(), torch.from_numpy(c)), (context, got.count.cpu(), c)
    assert torch.equal(got.start.cpu(), torch.from_numpy(s)), context
    assert torch.equal(got.end.cpu(), torch.from_numpy(e)), context
    assert torch.equal(got.score.cpu().view(torch.int32), torch.from_numpy(sc).view(torch.int32)), context      # bits, the -inf fill included
    if got.prob is not None:
        gp = got.prob.cpu().double().numpy()
        fill = np.arange(s.shape[1])[None, :] >= c[:, None]
        assert (gp[fill] == 0).all(), context                                                                   # a fill slot's prob is exactly 0
        if not gate_prob:
            return
        err = np.abs(gp - p) / (1e-4 * p + 1e-7)
        print('%s: prob error %.3f of the gate' % (context, float(err.max())))
        assert float(err.max()) <= 1.0, (context, float(err.max()))


@pytest.mark.gpu
@pytest.mark.parametrize('case', range(len(CASES)))
def test_exact_parity_with_the_specification(case):
    B, T, K, nms, span, kind = CASES[case]
    rng = np.random.default_rng(1000 + case)
    lengths = _lengths(rng, kind, B, T)
    for clip in (False, True):                                   # 3 N(0, 1) as it comes: exact spans and scores ; clipped to |x| <= 8: `prob` gated as well
        sl, el = _logits(rng, B, T, lengths, clip=clip)
        _assert_exact(_run(sl, el, K, nms, span, lengths), topk_spans_reference(sl, el, K, nms, span, lengths), (CASES[case], clip), gate_prob=clip)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [33, 257])
def test_a_max_span_at_or_beyond_the_length_limits_nothing(T):
    """max_span >= T, up to the largest int, is "no limit": the same spans as max_span = 0, and the specification's"""
    rng = np.random.default_rng(1500 + T)
    lengths = np.array([T, max(1, T - 9), 1], dtype=np.int64)
    sl, el = _logits(rng, 3, T, lengths)
    free = _run(sl, el, 32, 0.5, 0, lengths)
    for span in (T - 1, T, T + 5, 2 ** 31 - 256, 2 ** 31 - 1):
        got = _run(sl, el, 32, 0.5, span, lengths)
        _assert_exact(got, topk_spans_reference(sl, el, 32, 0.5, span, lengths), ('max_span', T, span))
        if span >= T:
            assert all(torch.equal(a, b) for a, b in zip(got, free)), span


def test_the_parity_cases_cover_what_they_must():
    for col, want in ((0, {1, 3, 64}), (1, {1, 2, 3, 31, 32, 33, 117, 255, 256, 257, 511, 1024}), (2, {1, 5, 32}), (3, {1.0, 0.5, 0.0}), (4, {0, 1, 7}),
                      (5, {'none', 'ragged', 'edge'})):
        assert {c[col] for c in CASES} == want
    with_nms = [c for c in CASES if c[3] < 1.0]
    assert {c[4] for c in with_nms} == {0, 1, 7} and {c[5] for c in with_nms} == {'none', 'ragged', 'edge'}      # every option together with NMS


@pytest.mark.gpu
@pytest.mark.parametrize('T,nms', [(64, 1.0), (64, 0.5), (300, 1.0), (300, 0.5)])
def test_ties_follow_the_order_rule(T, nms):
    """integer logits -2 .. 2: the sums tie massively, so the result pins start-then-end order and the rescans"""
    rng = np.random.default_rng(2000 + T)
    lengths = np.array([T, max(1, T - 7)], dtype=np.int64)
    sl, el = _logits(rng, 2, T, lengths, integers=True)
    _assert_exact(_run(sl, el, 32, nms, 0, lengths), topk_spans_reference(sl, el, 32, nms, 0, lengths), ('ties', T, nms))


@pytest.mark.gpu
def test_exhaustion_fills_the_documented_values():
    for T, nms in ((3, 1.0), (5, 0.5), (257, 0.0)):
        rng = np.random.default_rng(3000 + T)
        sl, el = _logits(rng, 2, T, None)
        got, ref = _run(sl, el, 32, nms, 0, None), topk_spans_reference(sl, el, 32, nms, 0, None)
        _assert_exact(got, ref, ('exhaustion', T, nms))
        c = got.count.cpu().numpy()
        assert (c >= 1).all() and (T > 5 or (c < 32).all())      # (T = 3: 6 candidates, T = 5: 15 -- fewer than K)
        for b in range(2):
            assert (got.start[b, c[b]:] == -1).all() and (got.end[b, c[b]:] == -1).all() and torch.isneginf(got.score[b, c[b]:]).all()
            assert (got.prob[b, c[b]:] == 0).all()
    assert (_run(sl, el, 32, 1.0, 0, None, want_prob=False).prob is None)


@pytest.mark.gpu
def test_long_video():
    """T = 4096: the LDS budget and the 16-bit end cache up to index 4095"""
    rng = np.random.default_rng(4096)
    lengths = np.array([4096, 3001], dtype=np.int64)
    sl, el = _logits(rng, 2, 4096, lengths)
    el[0, 4095] = 8.0                                            # the last clip is an end worth choosing
    _assert_exact(_run(sl, el, 3, 0.5, 0, lengths), topk_spans_reference(sl, el, 3, 0.5, 0, lengths), 'T 4096')


@pytest.mark.gpu
def test_prob_of_all_candidates_is_the_upper_triangular_mass():
    """T = 5, K = 32, no NMS, no length: all 15 candidates come back, so their probabilities add up to the mass softmax(sl) softmax(el)^T puts on s <= e
    (the two softmaxes together sum to 1 over the FULL square; the part below the diagonal is not a candidate)"""
    rng = np.random.default_rng(5)
    sl, el = _logits(rng, 4, 5, None)
    got = _run(sl, el, 32, 1.0, 0, None)
    assert (got.count.cpu() == 15).all()
    ps, pe = (torch.softmax(torch.from_numpy(x).double(), dim=1) for x in (sl, el))
    mass = torch.triu(ps[:, :, None] * pe[:, None, :]).sum(dim=(1, 2))
    total = got.prob.cpu().double().sum(dim=1)
    print('sum of prob - mass:', (total - mass).abs().max().item())
    assert float((total - mass).abs().max()) <= 1e-5 and (total <= 1.0 + 1e-5).all()


@pytest.mark.gpu
def test_top1_agrees_with_extract_index_on_the_device():
    eng, dropped, n = _engine(), 0, 0
    for seed in range(200):
        sl, el = _seeded_case(seed)
        ps, pe = torch.softmax(torch.from_numpy(sl).double(), 1)[0], torch.softmax(torch.from_numpy(el).double(), 1)[0]
        joint = torch.triu(ps[:, None] * pe[None, :]).reshape(-1).sort(descending=True).values
        n += 1
        if joint.numel() > 1 and not (joint[0] - joint[1]) > 1e-6 * joint[0]:
            dropped += 1                                         # best and second best too close for the product form of k_extract_index
            continue
        dsl, del_ = torch.from_numpy(sl).cuda(), torch.from_numpy(el).cuda()
        si, ei = eng.extract_index(dsl, del_)
        top = eng.extract_topk(dsl, del_, 1, nms_iou=1.0)
        assert int(top.count[0]) == 1 and int(top.start[0, 0]) == int(si[0]) and int(top.end[0, 0]) == int(ei[0]), seed
    assert dropped <= 0.05 * n, (dropped, n)


@pytest.mark.gpu
def test_misuse_is_refused_by_name_and_the_next_call_works():
    from vslnet_amd.engine import VslError
    eng = _engine()
    rng = np.random.default_rng(6)
    sl, el = (torch.from_numpy(x).cuda() for x in _logits(rng, 3, 40, None))
    good = eng.extract_topk(sl, el, 5, nms_iou=0.5)
    mask = torch.ones(3, 40, device='cuda')

    def again():
        out = eng.extract_topk(sl, el, 5, nms_iou=0.5)
        assert all(torch.equal(a, b) for a, b in zip(out, good))
    for kw, exc, text in ((dict(k=0), VslError, 'K=0'), (dict(k=33), VslError, 'K=33'), (dict(k=5, nms_iou=1.5), VslError, 'nms_iou=1.5'),
                          (dict(k=5, max_span=-1), VslError, 'max_span=-1'), (dict(k=5, lengths=[40, 40, 40], v_mask=mask), ValueError, 'not both')):
        with pytest.raises(exc, match=text):
            eng.extract_topk(sl, el, **kw)
        again()
    for kw in (dict(k=5, max_span=2 ** 32), dict(k=5, max_span=2 ** 31), dict(k=2 ** 32 + 5)):      # (would wrap in a C int: 2 ** 32 to 0 = unlimited)
        with pytest.raises(ValueError, match='not a C int'):
            eng.extract_topk(sl, el, **kw)
    again()
    big = torch.zeros(1, 4097, device='cuda')
    with pytest.raises(VslError, match='T=4097'):
        eng.extract_topk(big, big, 1)
    again()
    with pytest.raises(ValueError, match='start_logits'):
        eng.extract_topk(torch.zeros(3, 80, device='cuda')[:, ::2], el, 5)          # not contiguous
    with pytest.raises(ValueError, match='end_logits'):
        eng.extract_topk(sl, el.double(), 5)
    again()
    eng.has_topk = False                                         # an older library: refused by name, no host fallback
    try:
        with pytest.raises(VslError, match='vsl_extract_topk is missing'):
            eng.extract_topk(sl, el, 5)
    finally:
        eng.has_topk = True
    again()
    # v_mask gives the lengths by its row sums
    lens = torch.tensor([40, 13, 1], device='cuda')
    m = (torch.arange(40, device='cuda')[None, :] < lens[:, None]).float()
    assert all(torch.equal(a, b) for a, b in zip(eng.extract_topk(sl, el, 5, nms_iou=0.5, v_mask=m), eng.extract_topk(sl, el, 5, nms_iou=0.5, lengths=lens)))


@pytest.mark.gpu
def test_two_calls_and_a_side_stream_give_the_same_bits():
    eng = _engine()
    rng = np.random.default_rng(7)
    lengths = np.array([300, 211, 5], dtype=np.int64)
    sl, el = (torch.from_numpy(x).cuda() for x in _logits(rng, 3, 300, lengths))
    a = eng.extract_topk(sl, el, 32, nms_iou=0.5, lengths=lengths)
    b = eng.extract_topk(sl, el, 32, nms_iou=0.5, lengths=lengths)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = eng.extract_topk(sl, el, 32, nms_iou=0.5, lengths=lengths)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.gpu
def test_the_call_leaves_the_handles_state_alone(monkeypatch):
    """One engine: a training step that meets the oracle (tests/helpers: logits, losses, every gradient, the saved activations the ReLU check reads);
    then extract_topk after an inference forward and after a localize; then the same step again with an extract_topk between its forward and its
    backward.  The second step meets the oracle too and leaves the bits of the first: the saved activation `gated` and the whole gradient."""
    from tests.helpers import check_training_against_oracle
    from vslnet_amd import engine as E
    B, T, Lq, Lc = 4, 96, 9, 6
    real, made, calls = E.Engine, [], []

    def same_engine(cfg, *a, **k):
        if not made:
            made.append(real(cfg, *a, **k))
        return made[0]
    monkeypatch.setattr(E, 'Engine', same_engine)
    step = dict(cfg=dict(video_feature_dim=64), lazy=True)
    before = check_training_against_oracle(B, T, Lq, Lc, context='before extract_topk', **step)
    eng = before.eng
    gated = eng.ws_view('gated', (B, T, 128)).clone()
    P, d = before.P, before.d
    pad, glove = P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda()
    _, sl, el = eng.forward(before.flat, pad, glove, d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], inference=True)
    calls.append(eng.extract_topk(sl, el, 5, nms_iou=0.5, v_mask=d['v_mask']))
    enc = eng.encode_video(before.flat, d['vfeats'][:3], d['v_mask'][:3])
    _, sl, el = eng.localize(before.flat, pad, glove, enc, [0, 2, 2, 1], d['word_ids'], d['char_ids'], d['q_mask'])
    calls.append(eng.extract_topk(sl, el, 5, nms_iou=0.5))
    forward = eng.forward

    def forward_then_topk(*a, **k):
        out = forward(*a, **k)
        calls.append(eng.extract_topk(out[1], out[2], 32, nms_iou=0.0))      # between the training forward and its backward
        return out
    monkeypatch.setattr(eng, 'forward', forward_then_topk)
    after = check_training_against_oracle(B, T, Lq, Lc, context='after extract_topk', **step)
    assert len(made) == 1 and after.eng is eng and len(calls) >= 3 and all(int(t.count.min()) >= 1 for t in calls)
    assert torch.equal(eng.ws_view('gated', (B, T, 128)), gated) and torch.equal(after.g, before.g)


def _eval_setup():
    from model.VSLNet import VSLNet
    from vslnet_amd.data import ResidentSplit, get_test_loader, synthetic_dataset
    from vslnet_amd.synthetic import make_configs
    configs = make_configs(video_feature_dim=64, max_pos_len=40, word_size=200, char_size=30, batch_size=8, drop_rate=0.2)
    dataset, feats = synthetic_dataset(configs, n_train=8, n_test=24, seed=3)
    torch.manual_seed(5)
    m = VSLNet(configs, dataset['word_vector']).to('cuda').eval()
    return m, get_test_loader(dataset['test_set'], feats, configs), ResidentSplit(dataset['test_set'], feats, configs, 'cuda', train=False)


@pytest.mark.gpu
@pytest.mark.parametrize('shared', [False, True])
def test_eval_loops_report_rank_at_k(shared, monkeypatch):
    m, loader, split = _eval_setup()
    fn, src = (runner.eval_test_shared, split) if shared else (runner.eval_test, loader)
    records = split.records if shared else [r for batch in loader for r in batch[0]]
    plain = fn(m, src, 'cuda', epoch=1, global_step=1)
    seen = []
    real = m.extract_topk

    def spy(sl, el, k, **kw):
        L = kw['lengths'] if kw.get('lengths') is not None else kw['v_mask'].sum(dim=1)
        seen.append((sl.cpu().numpy(), el.cpu().numpy(), L.cpu().numpy().astype(np.int64), k, kw['nms_iou'], kw['max_span']))
        return real(sl, el, k, **kw)
    monkeypatch.setattr(m, 'extract_topk', spy)
    got = fn(m, src, 'cuda', epoch=1, global_step=1, topk=TopK(5, 0.5, 0))
    assert len(plain) == 5 and len(got) == 6
    assert got[:4] == plain[:4] and got[4].startswith(plain[4]) and got[4][len(plain[4]):].startswith('Rank@5, IoU=0.3: ')
    best, n = [], 0
    for sl, el, L, k, nms, span in seen:
        assert (k, nms, span) == (5, 0.5, 0) and sl.shape[1] <= 40
        s, e, _, _, c = topk_spans_reference(sl, el, k, nms, span, L)
        for b in range(sl.shape[0]):
            best.append(runner.best_iou_of_spans(s[b], e[b], c[b], records[n]))
            n += 1
    assert n == len(records) == 24
    assert got[5] == runner.summarise_topk(best, 5)[0]
    assert all(got[5][k] >= v for k, v in zip(('r_k_i3', 'r_k_i5', 'r_k_i7', 'mIoU_k'), plain[:4]))
