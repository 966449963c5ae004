"""The video ranking loss, the written specification (CPU): the header's declarations and the library's exports, vslnet_amd.spans.group_loss_reference
-- what tests/test_group_loss.py compares the device with -- against torch autograd on a formula that shares no code with it, the sampler
ResidentSplit.shards(negatives=n) on a CPU-resident split, and every refusal of main.py's --rank_* flags."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, header_fields
from vslnet_amd.spans import group_loss_reference, pair_relevance_reference


def _header():
    return open(os.path.join(ROOT, 'include', 'vslnet_hip.h')).read()


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_declares_the_group_loss_and_keeps_abi_9():
    from vslnet_amd import engine
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    assert re.search(r'int vsl_group_loss\(vsl_handle h, const vsl_group_loss_io\* l, void\* hip_stream\);', src)
    assert re.search(r'int vsl_group_loss_scratch_floats\(int B, int G, int64_t\* out\);', src)
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', src) and engine.ABI_VERSION == 9      # an added entry point does not move the version
    names = header_fields('vsl_group_loss_io')
    assert names == [f[0] for f in engine.vsl_group_loss_io._fields_]                          # the ctypes mirror follows the header's field order
    assert names[:3] == ['B', 'T', 'G'] and names[-1] == 'scratch' and len(names) == 27
    # three int32, then 9 pointers (aligned at 16), 7 floats + 1 int32, 7 pointers
    assert ctypes.sizeof(engine.vsl_group_loss_io) == 16 + 9 * 8 + 8 * 4 + 7 * 8


def test_library_exports_the_group_loss():
    from vslnet_amd import build, engine
    lib = ctypes.CDLL(build.build())
    for s in ('vsl_group_loss', 'vsl_group_loss_scratch_floats'):
        assert hasattr(lib, s), s
        assert s in engine.ABI_SYMBOLS, s
    assert lib.vsl_abi_version() == 9
    assert 'kernels_group_loss.hip' in build.SOURCES
    lib.vsl_group_loss_scratch_floats.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    lib.vsl_last_error.restype = ctypes.c_char_p
    n = ctypes.c_int64()
    assert lib.vsl_group_loss_scratch_floats(12, 4, ctypes.byref(n)) == 0 and n.value >= 10 * 12
    assert lib.vsl_group_loss_scratch_floats(3, 4, ctypes.byref(n)) != 0 and b'G=4' in lib.vsl_last_error()
    assert lib.vsl_group_loss_scratch_floats(0, 1, ctypes.byref(n)) != 0 and b'B=0' in lib.vsl_last_error()


# ------------------------------------------------------------------------------------------------ the specification against autograd
def spec_case(T, sizes=(1, 2, 4, 5), seed=0, tie=True):
    """B = sum(sizes) rows in groups of `sizes`, ragged masks (no prefix on one row), the positive somewhere inside its group.  With four groups or
    more: row 1 (a negative of group 1) is fully masked, group 2's POSITIVE row is fully masked (the group is skipped), and with `tie` and T >= 3
    the positive row of the last group attains its maximum at two valid clips."""
    rng = np.random.RandomState(seed)
    B = int(sum(sizes))
    gs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pos = np.array([gs[g] + rng.randint(sizes[g]) for g in range(len(sizes))], dtype=np.int32)
    h = rng.uniform(0.02, 0.98, size=(B, T)).astype(np.float32)
    lens = rng.randint(max(1, T // 2), T + 1, size=B)
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)
    if T >= 4:
        mask[0, 1] = 0.0                                                      # a mask that is no prefix
    if len(sizes) >= 4:
        if pos[1] == 1:
            pos[1] = 2
        mask[1] = 0.0                                                         # a fully masked NEGATIVE row: out of its group's softmax
        mask[pos[2]] = 0.0                                                    # a fully masked POSITIVE row: its group is skipped
        if tie and T >= 3:
            b = pos[-1]
            mask[b, :3] = 1.0
            h[b, 0], h[b, 2] = 0.99, 0.99                                     # the gradient lands on clip 0
    sl, el = rng.randn(B, T).astype(np.float32) * 2, rng.randn(B, T).astype(np.float32) * 2
    s_lab, e_lab = rng.randint(0, T, size=B).astype(np.int64), rng.randint(0, T, size=B).astype(np.int64)
    h_lab = (rng.uniform(size=(B, T)) < 0.3).astype(np.int64)
    is_pos = np.zeros(B, dtype=bool)
    is_pos[pos] = True
    h_lab[~is_pos] = 0
    return dict(h=h, sl=sl, el=el, mask=mask, s_lab=s_lab, e_lab=e_lab, h_lab=h_lab, gs=gs, pos=pos)


def torch_formula(c, mode, tau, w_loc, w_hl, w_rank):
    """loc, hl, rank, total and d total / d (h, sl, el) by autograd in float64: amax / mean / logsumexp, CrossEntropy and BCE from torch.nn.functional"""
    F = torch.nn.functional
    h = torch.tensor(c['h'], dtype=torch.float64, requires_grad=True)
    sl = torch.tensor(c['sl'], dtype=torch.float64, requires_grad=True)
    el = torch.tensor(c['el'], dtype=torch.float64, requires_grad=True)
    m = torch.tensor(c['mask'], dtype=torch.float64)
    G, pos = len(c['pos']), torch.tensor(c['pos'], dtype=torch.int64)
    loc = (F.cross_entropy(sl[pos], torch.tensor(c['s_lab'])[pos], reduction='sum') + F.cross_entropy(el[pos], torch.tensor(c['e_lab'])[pos], reduction='sum')) / G
    y = torch.tensor(c['h_lab'], dtype=torch.float64)
    w = torch.where(y == 0, torch.ones_like(y), 2.0 * y)
    hl = (F.binary_cross_entropy(h, y, reduction='none') * w * m).sum() / (m.sum() + 1e-12)
    inv_t = float(np.float32(1.0 / tau))
    rank, hits = torch.zeros((), dtype=torch.float64), 0
    for g in range(G):
        rows = [b for b in range(c['gs'][g], c['gs'][g + 1]) if c['mask'][b].any()]
        p = int(c['pos'][g])
        if p not in rows:
            continue
        valid = [torch.tensor(np.flatnonzero(c['mask'][b])) for b in rows]
        r = torch.stack([torch.amax(h[b][v]) if mode == 'max' else torch.mean(h[b][v]) for b, v in zip(rows, valid)])
        z = r * inv_t
        rank = rank + torch.logsumexp(z, 0) - z[rows.index(p)]
        zd = z.detach().numpy()
        hits += int(all(zd[rows.index(p)] > zd[i] or (zd[rows.index(p)] == zd[i] and p <= b) for i, b in enumerate(rows)))
    rank = rank / G
    total = w_loc * loc + w_hl * hl + w_rank * rank
    total.backward()
    return [float(x.detach()) for x in (loc, hl, rank, total)], hits, h.grad.numpy(), sl.grad.numpy(), el.grad.numpy()


@pytest.mark.parametrize('mode', ['max', 'mean'])
@pytest.mark.parametrize('tau', [1.0, 0.05])
@pytest.mark.parametrize('T', [1, 7, 33])
def test_group_loss_reference_against_autograd(mode, tau, T):
    c = spec_case(T, seed=T)
    got = group_loss_reference(c['h'], c['sl'], c['el'], c['mask'], c['s_lab'], c['e_lab'], c['h_lab'], c['gs'], c['pos'], 1.0, 5.0, 0.7, tau, mode)
    want, hits, d_h, d_sl, d_el = torch_formula(c, mode, tau, 1.0, 5.0, 0.7)
    # the specification's relevance is the device's float32 value (pair_relevance_reference(fp32_order=True)); autograd's is float64: the mean differs
    # by the float32 rounding of a sum of at most 33 terms in (0, 1), a few 1e-7, which 1 / tau = 20 scales up in z -- hence 2e-5; max is exact
    tol = 1e-9 if mode == 'max' else 2e-5
    assert got.hits == hits
    assert np.allclose(got.losses[:4], want, rtol=tol, atol=tol), (got.losses, want)
    assert got.losses[4] == c['mask'].sum()
    if mode == 'max' and T >= 3:
        # the two-clip tie: torch.amax hands each of the tied clips HALF of the gradient, the specification all of it to the first
        # (test_rank_gradient_alone_...); the sum over the two clips is the same
        b = c['pos'][-1]
        assert np.isclose(got.d_h[b, 0] + got.d_h[b, 2], d_h[b, 0] + d_h[b, 2], rtol=1e-9) and got.d_h[b, 0] != d_h[b, 0]
        d_h[b, [0, 2]] = got.d_h[b, [0, 2]]
    assert np.allclose(got.d_h, d_h, rtol=tol, atol=tol * max(1.0, np.abs(d_h).max()))
    assert np.allclose(got.d_sl, d_sl, rtol=1e-9, atol=1e-12) and np.allclose(got.d_el, d_el, rtol=1e-9, atol=1e-12)
    is_pos = np.zeros(len(c['h']), dtype=bool)
    is_pos[c['pos']] = True
    assert not got.d_sl[~is_pos].any() and not got.d_el[~is_pos].any()
    assert np.array_equal(got.relevance, pair_relevance_reference(c['h'], c['mask'], mode, fp32_order=True))
    assert np.isneginf(got.relevance[1]) and np.isneginf(got.relevance[c['pos'][2]])


def test_rank_gradient_alone_lands_on_the_first_maximum_and_skips_what_it_must():
    c = spec_case(7, seed=3)
    for mode in ('max', 'mean'):
        got = group_loss_reference(c['h'], c['sl'], c['el'], c['mask'], None, None, None, c['gs'], c['pos'], 0.0, 0.0, 1.0, 0.05, mode)
        want, hits, d_h, _, _ = torch_formula(c, mode, 0.05, 0.0, 0.0, 1.0)
        assert got.losses[0] == 0 and got.losses[1] == 0 and got.losses[3] == got.losses[2] and got.hits == hits
        b = c['pos'][-1]                                                      # the two-clip tie of the maximum (torch.amax halves it)
        if mode == 'max':
            assert np.isclose(d_h[b, 0], d_h[b, 2]) and np.isclose(got.d_h[b, 0], 2 * d_h[b, 0], rtol=1e-9)
            d_h[b, [0, 2]] = got.d_h[b, [0, 2]]
        assert np.allclose(got.d_h, d_h, rtol=2e-5, atol=2e-5 * np.abs(d_h).max())
        assert not got.d_h[c['mask'] == 0].any()                              # nothing under the mask
        assert not got.d_h[1].any()                                           # the fully masked negative row
        assert not got.d_h[c['gs'][2]:c['gs'][3]].any()                       # the skipped group: no rank gradient on any of its rows
        assert not got.d_h[0].any()                                           # a group of one: l = 0, d r = 0
        if mode == 'max':
            assert got.d_h[b, 0] != 0 and got.d_h[b, 2] == 0 and np.count_nonzero(got.d_h[b]) == 1
            assert (np.count_nonzero(got.d_h, axis=1) <= 1).all()
    with pytest.raises(ValueError, match='zero weight'):
        group_loss_reference(c['h'], c['sl'], c['el'], c['mask'], None, None, c['h_lab'], c['gs'], c['pos'], 1.0, 5.0)
    with pytest.raises(ValueError, match='non-empty groups'):
        group_loss_reference(c['h'], c['sl'], c['el'], c['mask'], None, None, None, [0, 3, 3, 12], [0, 3, 4], 0.0, 0.0)


def test_fp32_ordered_mean_is_the_butterfly_of_lane_partials():
    """pair_relevance_reference(fp32_order=True) against a scalar re-statement of the device's additions, and within float32 rounding of the fp64 mean"""
    rng = np.random.RandomState(1)
    for T in (1, 5, 64, 65, 257):
        h = rng.uniform(size=(3, T)).astype(np.float32)
        mask = (rng.uniform(size=(3, T)) < 0.8).astype(np.float32)
        mask[2] = 0
        got = pair_relevance_reference(h, mask, 'mean', fp32_order=True)
        for b in range(2):
            lanes = [np.float32(0)] * 64
            for t in range(T):
                if mask[b, t]:
                    lanes[t % 64] = np.float32(lanes[t % 64] + h[b, t])
            for step in (32, 16, 8, 4, 2, 1):
                lanes = [np.float32(lanes[i] + lanes[i ^ step]) for i in range(64)]
            n = int(mask[b].sum())
            if n:
                assert got[b] == np.float32(lanes[0] / np.float32(n))
        assert np.isneginf(got[2])
        assert np.allclose(got[:2], pair_relevance_reference(h, mask, 'mean')[:2], rtol=1e-6)
        assert np.array_equal(pair_relevance_reference(h, mask, 'max', fp32_order=True), pair_relevance_reference(h, mask, 'max'))


# ------------------------------------------------------------------------------------------------ the sampler
def _split(n_train=22, batch_size=16, seed=3):
    from vslnet_amd.data import ResidentSplit, synthetic_dataset
    cfg = SimpleNamespace(video_feature_dim=16, max_pos_len=32, word_dim=8, batch_size=batch_size)
    ds, feats = synthetic_dataset(cfg, n_train=n_train, n_test=2)
    return ResidentSplit(ds['train_set'], feats, cfg, 'cpu', train=True, generator=torch.Generator().manual_seed(seed))


def test_sampler_emits_one_group_per_record_with_the_positive_first():
    sp, n = _split(), 3
    steps = list(sp.shards(negatives=n))
    assert len(steps) == sp.steps_per_epoch(n) == -(-22 // 4) and len(sp) == 2          # ceil(records / P), P = 16 // 4; len() stays the plain count
    seen = []
    for b in steps:
        B, T = b['v_mask'].shape
        gs, pos, vi = b['group_start'].tolist(), b['positive'].tolist(), b['video_index'].tolist()
        assert B <= sp.batch_size and gs[0] == 0 and gs[-1] == B and len(pos) == len(gs) - 1 == b['n_pos']
        assert b['group_start'].dtype == b['positive'].dtype == b['video_index'].dtype == torch.int32
        N = b['vfeats'].shape[0]
        assert b['vfeats'].shape[1] == T == int(b['video_v_mask'].sum(1).max()) and b['video_v_mask'].shape == (N, T)
        assert torch.equal(b['v_mask'], b['video_v_mask'][b['video_index'].long()])
        assert b['lens_global'].tolist() == b['v_mask'].sum(1).long().tolist() and b['row0'] == 0
        for g in range(len(pos)):
            rows = list(range(gs[g], gs[g + 1]))
            assert pos[g] == rows[0] and len(rows) == 1 + min(n, N - 1)                 # positive first; every other video of the step at most once
            vids = [vi[r] for r in rows]
            assert len(set(vids)) == len(vids)                                          # without replacement, never the group's own video
            rec = b['records'][rows[0]]
            assert all(b['records'][r] is rec for r in rows)
            assert all(torch.equal(b['word_ids'][r], b['word_ids'][rows[0]]) and torch.equal(b['char_ids'][r], b['char_ids'][rows[0]]) for r in rows)
            assert int(b['s_labels'][rows[0]]) == rec['s_ind'] and int(b['e_labels'][rows[0]]) == rec['e_ind'] and int(b['h_labels'][rows[0]].sum()) > 0
            own = b['vfeats'][vids[0], :rec['v_len']]
            assert torch.equal(own, sp.feats[sp.vid_of[sp.records.index(rec)], :rec['v_len']])
            for r in rows[1:]:
                assert not b['h_labels'][r].any() and int(b['s_labels'][r]) == 0 and int(b['e_labels'][r]) == 0
            seen.append(rec['sample_id'])
    assert sorted(seen) == list(range(22))                                              # every record exactly once per epoch


def test_sampler_is_reproducible_and_ragged_when_videos_run_out():
    a, b = list(_split(seed=7).shards(negatives=3)), list(_split(seed=7).shards(negatives=3))
    c = list(_split(seed=8).shards(negatives=3))
    same = lambda x, y: all(torch.equal(p['video_index'], q['video_index']) and torch.equal(p['word_ids'], q['word_ids']) for p, q in zip(x, y))
    assert same(a, b) and not same(a, c)
    last = a[-1]                                                                        # 22 = 5 * 4 + 2: two records, two videos, n = 3
    assert last['n_pos'] == 2 and last['group_start'].tolist() == [0, 2, 4] and last['vfeats'].shape[0] == 2
    big = list(_split(n_train=3, batch_size=16).shards(negatives=7))                    # P = 2: a step of 2 videos, then one of a single video
    assert [s['group_start'].tolist() for s in big] == [[0, 2, 4], [0, 1]]


def test_sampler_refusals():
    sp = _split()
    for kw, word in ((dict(negatives=3, queries_per_video=2), 'queries_per_video'), (dict(negatives=3, micro_batches=2), 'micro_batches'),
                     (dict(negatives=3, world=2), 'world'), (dict(negatives=16), 'batch_size'), (dict(negatives=-1), 'at least 0')):
        with pytest.raises(ValueError, match=word):
            next(iter(sp.shards(**kw)))
    sp.train = False
    with pytest.raises(ValueError, match='train split'):
        next(iter(sp.shards(negatives=1)))


# ------------------------------------------------------------------------------------------------ the command line
@pytest.mark.parametrize('argv,word', [
    (['--rank_negatives', '3'], '--share_videos'),
    (['--rank_negatives', '3', '--share_videos', '--data', 'loader'], '--data resident'),
    (['--rank_negatives', '3', '--share_videos', '--optimizer', 'torch'], '--optimizer fused'),
    (['--rank_negatives', '3', '--share_videos', '--accum_steps', '2'], '--accum_steps 1'),
    (['--rank_negatives', '-1', '--share_videos'], 'at least 0'),
    (['--rank_negatives', '16', '--share_videos'], '--batch_size'),
    (['--rank_negatives', '3', '--share_videos', '--rank_temperature', '0'], '--rank_temperature'),
    (['--rank_lambda', '2.0'], '--rank_lambda needs --rank_negatives'),
    (['--rank_temperature', '0.2'], '--rank_temperature needs --rank_negatives'),
    (['--rank_relevance', 'mean'], '--rank_relevance needs --rank_negatives'),
])
def test_cli_refuses_by_name(argv, word):
    import main
    with pytest.raises(ValueError, match=re.escape(word)):
        main.run(['--task', 'synthetic', '--mode', 'train'] + argv)                     # (refused before the dataset is built or a device is asked for)


def test_cli_accepts_and_resolves_the_defaults():
    import main
    p = main.build_parser()
    assert main.rank_of(p.parse_args([])) is None
    assert main.rank_of(p.parse_args(['--share_videos', '--rank_negatives', '3'])) == (3, 1.0, 0.1, 'max')
    got = main.rank_of(p.parse_args(['--share_videos', '--rank_negatives', '2', '--rank_lambda', '0.5', '--rank_temperature', '0.2', '--rank_relevance', 'mean']))
    assert got == (2, 0.5, 0.2, 'mean')
    # --mode test reads what the run stored: the training-only requirements do not apply there
    assert main.rank_of(p.parse_args(['--mode', 'test', '--rank_negatives', '3', '--data', 'loader'])) == (3, 1.0, 0.1, 'max')
    stored = vars(p.parse_args(['--share_videos', '--rank_negatives', '3']))
    assert {'rank_negatives', 'rank_lambda', 'rank_temperature', 'rank_relevance'} <= set(stored)      # like every flag: into configs.json
