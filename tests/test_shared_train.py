"""Training through a shared video encoding: vsl_forward_shared + vsl_backward_shared, Engine / VSLNet.forward_shared,
ResidentSplit.shards(queries_per_video=K), main.py --mode train --share_videos.

A step over N videos and B queries, query b paired with video video_index[b]: VisualProjection and encoder application 0 run forward and backward on
N T rows, everything else on B samples; the gradient of the encoding is summed over each video's queries in ascending b (no atomics).

CPU: the ABI (exports, version 9, vsl_io unmoved, the ctypes mirror of vsl_shared_io), the oracle restatement `oracle_train_shared` the GPU numbers
are gated against (at drop_rate 0 it IS O.total_loss on the replicated batch; it makes the oracle's 41 / 23 dropout calls) and the grouped order.
GPU: training parity against the restatement on the HIP path's own dropout masks (the video sites draw (N, ...) shapes: one mask per video) and its
ReLU branches, at the project's gates; equality with the ordinary step on the replicated batch at drop_rate 0; determinism; the workspace bound;
loud failures on misuse; the module and the training loop."""
import ctypes
import json
import os
import re
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import (HIP_DROP_SITES, ROOT, assert_forced_relu_inside_noise, check_training_against_oracle, grad_tol, header_fields, header_sizeof,
                           hip_dropout)

NEW_SYMBOLS = ('vsl_shared_workspace_floats', 'vsl_forward_shared', 'vsl_backward_shared', 'vsl_shared_workspace_offset')
SIZEOF_VSL_IO = 208             # ABI 9, `inference` last: the struct must not move
STEP_SEED = (7 << 33) + 12345   # (exercises the high word of the 64-bit seed too)


# ------------------------------------------------------------------------------------------------ 1. the ABI (CPU)
def _header():
    return open(os.path.join(ROOT, 'include', 'vslnet_hip.h')).read()


def test_library_exports_the_shared_training_entry_points_and_keeps_abi_9():
    from vslnet_amd import build, engine
    lib = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in engine.ABI_SYMBOLS, s
        assert re.fullmatch(r'vsl_[a-z_]+', s)
    assert lib.vsl_abi_version() == 9 == engine.ABI_VERSION
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', _header())
    # (the mirror of vsl_shared_io against the host compiler's layout: tests/test_abi_layout.py, as for every struct)
    assert ctypes.sizeof(engine.vsl_io) == header_sizeof('vsl_io') == SIZEOF_VSL_IO and header_fields('vsl_io')[-1] == 'inference'
    assert header_fields('vsl_shared_io') == [f[0] for f in engine.vsl_shared_io._fields_] == ['N', 'video_index', 'video_v_mask']


# ------------------------------------------------------------------------------------------------ 2. the oracle, restated (CPU)
def oracle_train_shared(P, cfg, sb, training=True, highlight_lambda=5.0):
    """O.total_loss with the video half hoisted, in O.forward's call order (projection, embedding, video encoder, query encoder, CQ, predictor): the N
    videos go through VisualProjection and the feature encoder ONCE, the encoding and the mask are index_select-ed per query, everything else is
    O.forward's own sequence on B samples.  The dropout calls keep the oracle's numbering (helpers.HIP_DROP_SITES applies unchanged); the calls of
    the video half draw (N, ...) shapes.  The oracle itself is not edited.  -> (total, (h, sl, el, hl, loc))."""
    p, H = float(cfg.drop_rate), int(cfg.num_heads)
    idx = torch.as_tensor(sb['idx'], dtype=torch.int64)
    vf = O.visual_projection(P, sb['vfeats'], p, training)
    qf = O.embedding(P, sb['word_ids'], sb['char_ids'], p, training)
    enc = O.feature_encoder(P, 'feature_encoder.', vf, sb['video_v_mask'], H, p, training, None)
    qe = O.feature_encoder(P, 'feature_encoder.', qf, sb['q_mask'], H, p, training, None)
    ve, vm = torch.index_select(enc, 0, idx), torch.index_select(sb['video_v_mask'], 0, idx)
    f1 = O.cq_attention(P, ve, qe, vm, sb['q_mask'], p, training, None)
    f2 = O.cq_concat(P, f1, qe, sb['q_mask'])
    h = O.highlight(P, f2, vm)
    sl, el = O.conditioned_predictor(P, f2 * h[:, :, None], vm, cfg.predictor, H, p, training, None)
    hl = O.highlight_loss(h, sb['h_labels'], vm)
    loc = O.span_loss(sl, el, sb['s_labels'], sb['e_labels'])
    return loc + highlight_lambda * hl, (h, sl, el, hl, loc)


def shared_batch(cfg, N, idx, T, Lq, Lc, seed, extreme=False):
    """N videos (features, lengths, mask; video 0 fills T) and B = len(idx) queries drawn independently, labels inside each query's own video.
    extreme: the last video shrinks to ONE clip and the first query to ONE word.  -> dict with the per-video tensors (vfeats (N, T, Dv),
    video_v_mask (N, T)), the per-query tensors (v_mask = video_v_mask[idx] included) and `idx`."""
    idx = list(idx)
    B = len(idx)
    assert min(idx) >= 0 and max(idx) < N
    vb = O.synthetic_batch(cfg, N, T, Lq, Lc, seed=seed, ragged=N > 1)
    qb = O.synthetic_batch(cfg, B, T, Lq, Lc, seed=seed + 1, ragged=B > 1)
    vfeats, vlens = vb['vfeats'].clone(), vb['lens'].clone()
    word_ids, char_ids = qb['word_ids'].clone(), qb['char_ids'].clone()
    if extreme:
        vfeats[-1, 1:] = 0.0
        vlens[-1] = 1
        word_ids[0, 1:] = 0
        char_ids[0, 1:] = 0
    vmask = O.convert_length_to_mask(vlens)
    assert vmask.shape == (N, T) and int(vlens[0]) == T
    lens = vlens[idx]
    g = torch.Generator().manual_seed(seed + 2)
    s = (torch.rand(B, generator=g) * (lens.float() / 2)).long()
    e = torch.minimum(s + (torch.rand(B, generator=g) * (lens.float() / 8 + 1)).long(), lens - 1)
    return dict(vfeats=vfeats, video_v_mask=vmask, idx=idx, lens=lens, v_mask=vmask[idx], word_ids=word_ids, char_ids=char_ids,
                q_mask=(word_ids != 0).float(), s_labels=s, e_labels=e, h_labels=O.highlight_labels(s, e, lens, T))


def replicated(sb):
    """the ordinary batch the shared step stands for: features and mask gathered per query"""
    b = {k: sb[k] for k in ('lens', 'v_mask', 'word_ids', 'char_ids', 'q_mask', 's_labels', 'e_labels', 'h_labels')}
    b['vfeats'] = sb['vfeats'][sb['idx']]
    return b


@pytest.mark.parametrize('predictor', ['transformer', 'rnn'])
def test_oracle_restatement_equals_the_total_loss_on_the_replicated_batch(predictor):
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=64, word_size=102, predictor=predictor)
    P = O.random_params(cfg, seed=11)
    sb = shared_batch(cfg, 3, [0, 0, 2, 1, 0, 2, 2], 40, 9, 6, seed=12)
    grads = []
    for fn in (lambda Pg: oracle_train_shared(Pg, cfg, sb, training=True), lambda Pg: O.total_loss(Pg, cfg, replicated(sb), training=True)):
        Pg = {k: v.clone().requires_grad_(k not in O.FROZEN) for k, v in P.items()}
        total, (h, sl, el, hl, loc) = fn(Pg)
        total.backward()
        grads.append((total.detach(), hl.detach(), loc.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pg.items()}))
    (ta, ha, la, ga), (tb, hb, lb, gb) = grads
    for a, c in ((ta, tb), (ha, hb), (la, lb)):
        assert abs(float(a) - float(c)) <= 1e-6 * max(1.0, abs(float(c))), (float(a), float(c))
    for k in gb:
        if k in O.FROZEN:
            continue
        err = float((ga[k] - gb[k]).abs().max())
        assert err <= grad_tol(gb[k].numpy()), (k, err)
    # the dropout calls: the oracle's count and numbering, the video half's calls with (N, ...) shapes
    cfgd = O.make_cfg(video_feature_dim=64, max_pos_len=64, word_size=102, predictor=predictor, drop_rate=0.2)
    shapes = []

    def mask(call, shape, p):
        shapes.append(shape)
        return torch.ones(shape)
    try:
        O.force_dropout(mask)
        with torch.no_grad():
            oracle_train_shared(P, cfgd, sb, training=True)
        n_calls = O.DROP_CALLS
    finally:
        O.force_dropout(None)
    assert n_calls == (41 if predictor == 'transformer' else 23) == len(shapes)
    assert len(HIP_DROP_SITES) == 41
    for call, shape in enumerate(shapes):
        video_half = HIP_DROP_SITES[call] == 64 or HIP_DROP_SITES[call] < 16
        assert shape[0] == (3 if video_half else 7), (call, HIP_DROP_SITES[call], shape)


# ------------------------------------------------------------------------------------------------ 3. the grouped order (CPU)
@pytest.mark.parametrize('K', [1, 3, 4])
def test_grouped_order_covers_every_record_once_in_groups_of_at_most_k(K):
    from vslnet_amd import data
    cfg = SimpleNamespace(video_feature_dim=16, max_pos_len=24, word_dim=20, batch_size=16, seed=3)
    dataset, feats = data.synthetic_dataset(cfg, n_train=40, n_test=8, seed=3)
    recs = [dict(r) for r in dataset['train_set']]
    vids = sorted({r['vid'] for r in recs})[:9]
    for i, r in enumerate(recs):                                   # 40 queries over 9 videos: 4 or 5 per video
        r['vid'] = vids[i % len(vids)]
        L = feats[r['vid']].shape[0]
        r['s_ind'], r['e_ind'], r['v_len'] = min(r['s_ind'], L - 2), min(max(r['e_ind'], min(r['s_ind'], L - 2)), L - 1), L
    split = data.ResidentSplit(recs, feats, cfg, 'cpu', train=True, generator=torch.Generator().manual_seed(5))
    seen = Counter()
    nb = 0
    for b in split.shards(queries_per_video=K):
        nb += 1
        B, N = b['word_ids'].shape[0], b['vfeats'].shape[0]
        T = b['vfeats'].shape[1]
        assert b['video_index'].dtype == torch.int32 and b['video_index'].shape == (B,)
        assert b['video_v_mask'].shape == (N, T) and b['v_mask'].shape == (B, T)
        vi = b['video_index'].long()
        assert int(vi.min()) == 0 and int(vi.max()) == N - 1 and max(Counter(vi.tolist()).values()) <= K
        assert torch.equal(b['v_mask'], b['video_v_mask'][vi])
        if K == 1:
            assert N == B and vi.tolist() == list(range(B))
        for row, r in enumerate(b['records']):
            seen[r['sample_id']] += 1
            f = torch.from_numpy(feats[r['vid']])
            n = min(f.shape[0], T)
            got = b['vfeats'][vi[row]]
            assert torch.equal(got[:n], f[:n]) and not bool(got[n:].any()), 'video_index does not point at the row of the query\'s video'
            assert int(b['s_labels'][row]) == r['s_ind'] and int(b['v_mask'][row].sum()) == n
    assert nb == len(split) and sorted(seen) == sorted(r['sample_id'] for r in recs) and set(seen.values()) == {1}
    with pytest.raises(ValueError, match='single-process'):
        next(split.shards(1, 2, queries_per_video=K))


# ------------------------------------------------------------------------------------------------ 4. training parity against the restated oracle (GPU)
def hip_relu_masks_shared(eng, N, B, T, Lq, predictor):
    """helpers.hip_relu_masks for the plan of a shared step: the video pass' ReLU words have N T rows"""
    encs = [('venc', N, T)] * 4 + [('qenc', B, Lq)] * 4
    if predictor == 'transformer':
        encs += [('p1', B, T)] * 4 + [('p2', B, T)] * 4
    masks = []
    for k, (enc, n, L) in enumerate(encs):
        words = eng.ws_view('relu_%s_%d' % (enc, k % 4), (n * L * 4,)).view(torch.int32).cpu().view(n * L, 4)
        masks.append(((words.unsqueeze(-1) >> torch.arange(32, dtype=torch.int32)) & 1).bool().view(n, L, 128))
    for name in ('s', 'e'):
        masks.append(eng.ws_view('hid_' + name, (B, T, 128)).cpu() > 0)
    return masks


def _setup(N, idx, T, Lq, Lc=6, heads=8, predictor='transformer', Dv=64, drop_rate=0.2, extreme=False, param_seed=21, batch_seed=22):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg = O.make_cfg(video_feature_dim=Dv, max_pos_len=max(T, Lq), word_size=102, drop_rate=drop_rate, num_heads=heads, predictor=predictor)
    P = O.random_params(cfg, seed=param_seed)
    sb = shared_batch(cfg, N, idx, T, Lq, Lc, seed=batch_seed, extreme=extreme)
    d = {k: v.cuda().contiguous() for k, v in sb.items() if torch.is_tensor(v)}
    eng = Engine(cfg)
    return SimpleNamespace(cfg=cfg, P=P, sb=sb, d=d, eng=eng, flat=flat_from_state_dict(eng, P), pad=P['embedding_net.word_emb.pad_vec'].cuda(),
                           glove=P['embedding_net.word_emb.glove_vec'].cuda(), N=N, B=len(sb['idx']), T=T, Lq=Lq, Lc=Lc)


def _forward_shared(s, training=True, seed=STEP_SEED, flat=None, vfeats=None, eng=None):
    d = s.d
    return (eng or s.eng).forward_shared(s.flat if flat is None else flat, s.pad, s.glove, d['word_ids'], d['char_ids'], d['vfeats'] if vfeats is None else vfeats,
                                         d['video_v_mask'], d['q_mask'], s.sb['idx'], training=training, seed=seed)


def _step_shared(s, training=True, seed=STEP_SEED, lazy=False, eng=None, **kw):
    eng = eng or s.eng
    h, sl, el = _forward_shared(s, training, seed, eng=eng, **kw)
    d = s.d
    if lazy:
        losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0, inv_batch=1.0 / s.B, mask_sum=float(s.sb['v_mask'].sum()), lazy=True)
    else:
        losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
    return h, sl, el, losses, (d_h, d_sl, d_el)


def _oracle_on_hip_masks(s, sb, P, context):
    """the restated oracle on the HIP path's dropout masks and ReLU branches (the last forward of s.eng): -> (total, outputs, {name: grad})"""
    cfg = s.cfg
    try:
        O.force_dropout(hip_dropout(STEP_SEED))
        hip_masks = hip_relu_masks_shared(s.eng, s.N, s.B, s.T, s.Lq, cfg.predictor)
        O.force_relu_signs(hip_masks)
        Pg = {k: v.clone().requires_grad_(k not in O.FROZEN) for k, v in P.items()}
        total, outs = oracle_train_shared(Pg, cfg, sb, training=True)
        n_sites = O.DROP_CALLS
        O.force_relu_signs(None)
        O.force_dropout(None)
        if cfg.drop_rate > 0:
            assert n_sites == (41 if cfg.predictor == 'transformer' else 23), (context, n_sites)
        assert_forced_relu_inside_noise(O, context)
        total.backward()
    finally:
        O.force_relu_signs(None)
        O.force_dropout(None)
    return total.detach(), [t.detach() for t in outs], {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pg.items() if k not in O.FROZEN}


def _assert_parity(s, h, sl, el, losses, g, total, outs, ref, context):
    """the project's gates: logits 1e-4 * scale, h_score 2e-5, total loss 1e-4, every gradient 1e-4 * |g|inf + 1e-6, extract_index equal"""
    oh, osl, oel = outs[:3]
    fin = osl.abs() < 1e29
    scale = max(1.0, float(osl[fin].abs().max()))
    e_sl, e_el, e_h = float((sl.cpu() - osl)[fin].abs().max()), float((el.cpu() - oel)[fin].abs().max()), float((h.cpu() - oh).abs().max())
    e_t = abs(float(losses[2]) - float(total))
    print('[shared-train] %s: logits %.2e / %.2e (gate %.1e)  h_score %.2e (2e-5)  loss %.2e' % (context, e_sl, e_el, 1e-4 * scale, e_h, e_t))
    assert e_sl <= 1e-4 * scale and e_el <= 1e-4 * scale, context
    assert e_h <= 2e-5, context
    assert e_t <= 1e-4 * max(1.0, abs(float(total))), (context, float(losses[2]), float(total))
    bad, worst = [], 0.0
    for k, t in s.eng.views(g).items():
        err, tol = float((t.cpu() - ref[k]).abs().max()), 1e-4 * float(ref[k].abs().max()) + 1e-6
        if k == 'cq_attention.w4Q' and int(s.sb['q_mask'].sum(1).min()) == 1:
            tol = max(tol, 2e-5)            # a one-word query: that sample's share of dw4Q is a structural zero (helpers.check_training_against_oracle)
        worst = max(worst, err / tol)
        if not err <= tol:
            bad.append((k, err, tol))
    print('[shared-train] %s: worst gradient at %.3f of its gate' % (context, worst))
    assert not bad, (context, bad[:6])
    si, ei = s.eng.extract_index(sl, el)
    osi, oei = O.extract_index(osl, oel)
    assert torch.equal(si.cpu(), osi) and torch.equal(ei.cpu(), oei), context


def check_shared_against_oracle(context, N, idx, T, Lq, **kw):
    s = _setup(N, idx, T, Lq, **kw)
    h, sl, el, losses, seeds = _step_shared(s)
    g = s.eng.backward(*seeds, s.eng.new_flat()).clone()
    torch.cuda.synchronize()
    total, outs, ref = _oracle_on_hip_masks(s, s.sb, s.P, context)
    _assert_parity(s, h, sl, el, losses, g, total, outs, ref, context)
    return s, g


BASE = dict(N=3, idx=[0, 0, 2, 1, 0, 2, 2], T=64, Lq=9)
PARITY_CASES = [
    pytest.param(dict(BASE), id='base-grouping-with-repeats'),
    pytest.param(dict(N=2, idx=[0, 1, 0, 0, 1], T=117, Lq=20, extreme=True), id='off-tile-extreme'),
    pytest.param(dict(N=4, idx=[0, 1, 3, 3, 0, 1], T=96, Lq=9), id='unused-video'),
    pytest.param(dict(N=4, idx=[0, 1, 2, 3], T=64, Lq=9), id='N-equals-B'),
    pytest.param(dict(N=1, idx=[0] * 8, T=32, Lq=9), id='one-video'),
    pytest.param(dict(N=2, idx=[1, 0, 1], T=288, Lq=9), id='T288-streamed-attention'),
    pytest.param(dict(N=1, idx=[0, 0], T=1056, Lq=9), id='T1056-attn-dq'),
    pytest.param(dict(N=2, idx=[0, 1, 1, 0], T=64, Lq=33), id='Lq33-unfused-query-branch'),
    pytest.param(dict(N=2, idx=[0, 1, 1, 0, 1], T=64, Lq=9, heads=4), id='heads4'),
    pytest.param(dict(N=2, idx=[0, 1, 1, 0, 1], T=64, Lq=9, heads=1), id='heads1'),
    pytest.param(dict(N=2, idx=[1, 0, 1, 1], T=40, Lq=9, predictor='rnn'), id='rnn'),
]
WORKSPACE_SHAPES = [(c.values[0]['N'], len(c.values[0]['idx']), c.values[0]['T'], c.values[0]['Lq']) for c in PARITY_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize('c', PARITY_CASES)
def test_shared_step_matches_the_restated_oracle_on_the_same_dropout_masks(c, request):
    c = dict(c)
    s, g = check_shared_against_oracle(request.node.callspec.id, c.pop('N'), c.pop('idx'), c.pop('T'), c.pop('Lq'), **c)
    used = set(s.sb['idx'])
    if len(used) < s.N:
        # a video without a query: a zero dCv row, and nothing of it in the gradients (they met the oracle above, which never selects it)
        dcv = s.eng.ws_view('d_venc_video', (s.N, s.T, 128)).cpu()
        for n in range(s.N):
            assert bool((dcv[n] == 0).all()) == (n not in used), n
    # the grouping the backward summed over: ascending b inside every video
    start = s.eng.ws_view('group_start', (s.N + 1,)).view(torch.int32).cpu().tolist()
    members = s.eng.ws_view('group_members', (s.B,)).view(torch.int32).cpu().tolist()
    assert start[0] == 0 and start[-1] == s.B
    for n in range(s.N):
        assert members[start[n]:start[n + 1]] == [b for b, v in enumerate(s.sb['idx']) if v == n], (n, start, members)


@pytest.mark.gpu
def test_production_loss_and_fused_step_on_the_shared_step():
    """the base case through the production sequence: loss(lazy=True, inv_batch, mask_sum) -- inline seeds at T >= 32 -- and the optimizer step inside
    the backward.  The gradient meets the oracle; the parameters after the step are what vsl_adamw_step makes of that gradient."""
    from vslnet_amd.dp import FlatAdamW
    s = _setup(**BASE)
    flat = s.flat.clone()
    opt = FlatAdamW(flat, s.eng.layout, lr=1e-3, num_train_steps=10, clip_norm=0.05, engine=s.eng)
    s.eng.profile_select('*')
    try:
        h, sl, el, losses, seeds = _step_shared(s, lazy=True, flat=flat)
        fs = opt.fused_step()
        g = s.eng.backward(*seeds, s.eng.new_flat(), fused_step=fs)
        torch.cuda.synchronize()
        names = [r['name'] for r in s.eng.profile_launches()]
    finally:
        s.eng.profile_select(None)
    assert 'group_csr' in names and 'group_sum' in names and names.count('adamw') == 1, names
    assert names.index('loss') > names.index('head_bwd'), names            # the seeds were computed inline: the loss launch left the dependent chain
    total, outs, ref = _oracle_on_hip_masks(s, s.sb, s.P, 'production')
    _assert_parity(s, h, sl, el, losses, g, total, outs, ref, 'production')
    real = torch.zeros(s.eng.param_floats, dtype=torch.bool, device='cuda')
    for _, off, numel, _ in s.eng.layout:
        real[off:off + numel] = True
    want, m, v = s.flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
    s.eng.adamw_step(want, g, m, v, fs['lr'], fs['step'], clip_norm=0.05, norm_from_backward=True)
    torch.cuda.synchronize()
    assert not torch.equal(flat[real], s.flat[real])
    for x, y, nm in ((flat, want, 'params'), (opt.m, m, 'exp_avg'), (opt.v, v, 'exp_avg_sq')):
        assert torch.allclose(x[real], y[real], rtol=2e-5, atol=1e-8), (nm, float((x[real] - y[real]).abs().max()))     # (tests/test_optimizer.py's gate)


@pytest.mark.gpu
def test_bf16_features_on_the_shared_step():
    """bf16 throughput mode, base case, at the gates of tests/test_bf16_mode.py: against the oracle on the SAME rounded inputs (features and
    video_affine weight rounded to bf16) the parity gates apply."""
    s = _setup(**BASE)
    rnd = lambda t: t.to(torch.bfloat16).to(torch.float32)      # noqa: E731
    h, sl, el, losses, seeds = _step_shared(s, vfeats=s.d['vfeats'].to(torch.bfloat16))
    g = s.eng.backward(*seeds, s.eng.new_flat()).clone()
    torch.cuda.synchronize()
    Pr, sbr = dict(s.P), dict(s.sb)
    Pr['video_affine.linear.conv1d.weight'] = rnd(s.P['video_affine.linear.conv1d.weight'])
    sbr['vfeats'] = rnd(s.sb['vfeats'])
    total, outs, ref = _oracle_on_hip_masks(s, sbr, Pr, 'bf16')
    _assert_parity(s, h, sl, el, losses, g, total, outs, ref, 'bf16')


# ------------------------------------------------------------------------------------------------ 5. against the existing path (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize('N,B,T,Lq', [(3, 7, 64, 9), (2, 6, 128, 20)])
def test_shared_step_equals_the_ordinary_step_on_the_replicated_batch_at_drop_rate_0(N, B, T, Lq):
    idx = [0, 0, 2, 1, 0, 2, 2] if N == 3 else [1, 0, 0, 1, 1, 0]
    s = _setup(N, idx, T, Lq, drop_rate=0.0)
    d, eng = s.d, s.eng
    h, sl, el, losses, seeds = _step_shared(s)
    g = eng.backward(*seeds, eng.new_flat()).clone()
    outs = [t.clone() for t in (h, sl, el)]
    rep = d['vfeats'][torch.as_tensor(idx).cuda()].contiguous()
    h2, sl2, el2 = eng.forward(s.flat, s.pad, s.glove, d['word_ids'], d['char_ids'], rep, d['v_mask'], d['q_mask'], training=True, seed=STEP_SEED)
    _, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
    g2 = eng.backward(d_h, d_sl, d_el, eng.new_flat()).clone()
    torch.cuda.synchronize()
    for nm, a, c in zip(('h_score', 'start_logits', 'end_logits'), outs, (h2, sl2, el2)):
        assert torch.equal(a, c), '%s: max |diff| %g' % (nm, float((a - c).abs().max()))
    va, vb = eng.views(g), eng.views(g2)
    for k in vb:
        err = float((va[k] - vb[k]).abs().max())
        assert err <= 1e-4 * float(vb[k].abs().max()) + 1e-6, (k, err)


# ------------------------------------------------------------------------------------------------ 6. determinism (GPU)
@pytest.mark.gpu
def test_shared_step_is_bitwise_reproducible_across_engines_and_workspaces():
    from vslnet_amd.engine import Engine
    s = _setup(**BASE)
    runs = []
    for k in range(3):
        eng = s.eng
        if k == 2:                                     # a fresh engine; its workspace is allocated while the first one's is still alive
            eng = Engine(s.cfg)
        h, sl, el, losses, seeds = _step_shared(s, eng=eng)
        g = eng.backward(*seeds, eng.new_flat())
        torch.cuda.synchronize()
        runs.append(([t.clone() for t in (h, sl, el, losses, g)], eng._last_ws.data_ptr()))
    assert runs[2][1] != runs[0][1]
    for cur, _ in runs[1:]:
        for a, c in zip(runs[0][0], cur):
            assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ 7. workspace (GPU: plans need a device)
@pytest.mark.gpu
def test_shared_workspace_is_bounded_by_the_ordinary_plan():
    from vslnet_amd.engine import Engine
    engines = {}
    for c in PARITY_CASES:
        v = c.values[0]
        N, B, T, Lq = v['N'], len(v['idx']), v['T'], v['Lq']
        key = (v.get('heads', 8), v.get('predictor', 'transformer'), max(T, Lq))
        if key not in engines:
            engines[key] = Engine(O.make_cfg(video_feature_dim=64, max_pos_len=key[2], word_size=102, drop_rate=0.2, num_heads=key[0], predictor=key[1]))
        eng = engines[key]
        shared, plain = eng.shared_workspace_floats(B, N, T, Lq, 6), eng.workspace_floats(B, T, Lq, 6)
        print('[shared-train] workspace N=%d B=%d T=%d Lq=%d: %d floats = %.3f of the ordinary plan of B' % (N, B, T, Lq, shared, shared / plain))
        assert shared <= plain + N * T * 128 + B + N + 64, (N, B, T, Lq, shared, plain)
        if 2 * N <= B:
            assert shared < plain, (N, B, T, Lq, shared, plain)


# ------------------------------------------------------------------------------------------------ 8. misuse (GPU)
@pytest.mark.gpu
def test_misuse_fails_by_name_and_leaves_the_engine_usable():
    import ctypes as C
    from vslnet_amd.engine import VslError, vsl_shared_io, _ptr
    s = _setup(**BASE)
    eng, d = s.eng, s.d
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def err(rc):
        assert rc != 0
        return eng.lib.vsl_last_error().decode()
    h, sl, el, losses, seeds = _step_shared(s)
    io, sh = eng._last, eng._last_shared
    g = eng.new_flat()
    io.d_h_score, io.d_start_logits, io.d_end_logits, io.grads = _ptr(seeds[0]), _ptr(seeds[1]), _ptr(seeds[2]), _ptr(g)
    # vsl_backward on the saves of a shared forward
    assert 'vsl_backward:' in err(eng.lib.vsl_backward(eng.h, C.byref(io), stream)) and 'vsl_backward_shared' in eng.lib.vsl_last_error().decode()
    # N < 1, NULL index, NULL video mask -- in both calls
    for fn, name in ((eng.lib.vsl_forward_shared, 'vsl_forward_shared'), (eng.lib.vsl_backward_shared, 'vsl_backward_shared')):
        for field, value, word in (('N', 0, 'N=0'), ('video_index', None, 'video_index'), ('video_v_mask', None, 'video_v_mask')):
            bad = vsl_shared_io()
            C.memmove(C.byref(bad), C.byref(sh), C.sizeof(vsl_shared_io))
            setattr(bad, field, value)
            msg = err(fn(eng.h, C.byref(io), C.byref(bad), stream))
            assert name in msg and word in msg, msg
        for field, value, word in (('inference', 1, 'vsl_localize'), ('sample_offset', 3, 'sample_offset')):
            setattr(io, field, value)
            msg = err(fn(eng.h, C.byref(io), C.byref(sh), stream))
            setattr(io, field, 0)
            assert name in msg and word in msg, msg
    ev = torch.cuda.Event()
    ev.record()
    io.early_grads_event = C.c_void_p(ev.cuda_event)
    msg = err(eng.lib.vsl_backward_shared(eng.h, C.byref(io), C.byref(sh), stream))
    io.early_grads_event = None
    assert 'vsl_backward_shared' in msg and 'early_grads_event' in msg, msg
    # the refusals touched nothing: the backward of that forward still runs, twice the same
    g1 = eng.backward(*seeds, eng.new_flat()).clone()
    # vsl_backward_shared after an ordinary forward, and after an inference forward
    rep = d['vfeats'][torch.as_tensor(s.sb['idx']).cuda()].contiguous()
    for inference in (False, True):
        eng.forward(s.flat, s.pad, s.glove, d['word_ids'], d['char_ids'], rep, d['v_mask'], d['q_mask'], training=False, seed=0, inference=inference)
        msg = err(eng.lib.vsl_backward_shared(eng.h, C.byref(io), C.byref(sh), stream))
        assert 'vsl_backward_shared' in msg and 'last forward' in msg, msg
    # the Python layer: a host index out of range, the eval-only module call
    with pytest.raises(ValueError, match='out of range'):
        eng.forward_shared(s.flat, s.pad, s.glove, d['word_ids'], d['char_ids'], d['vfeats'], d['video_v_mask'], d['q_mask'], [0, 0, 3, 1, 0, 2, 2])
    with pytest.raises(VslError, match='inference forward'):
        eng.backward(*seeds, eng.new_flat())
    _step_shared(s)
    g2 = eng.backward(*eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)[1:], eng.new_flat())
    torch.cuda.synchronize()
    assert torch.equal(g1, g2)
    del eng, s
    # ... and an ordinary training step in an engine that has refused calls still meets the oracle
    r = check_training_against_oracle(4, 40, 9, 6, cfg=dict(video_feature_dim=64), context='ordinary step, fresh engine')
    sh0 = vsl_shared_io()
    assert r.eng.lib.vsl_backward_shared(r.eng.h, C.byref(r.eng._last), C.byref(sh0), stream) != 0
    dd = r.d
    r.eng.forward(r.flat, r.P['embedding_net.word_emb.pad_vec'].cuda(), r.P['embedding_net.word_emb.glove_vec'].cuda(), dd['word_ids'], dd['char_ids'],
                  dd['vfeats'], dd['v_mask'], dd['q_mask'], training=True, seed=(7 << 33) + 12345)
    _, d_h, d_sl, d_el = r.eng.loss(dd['s_labels'], dd['e_labels'], dd['h_labels'], 1.0, 5.0)
    g3 = r.eng.backward(d_h, d_sl, d_el, r.eng.new_flat())
    torch.cuda.synchronize()
    assert torch.equal(g3, r.g)               # the step check_training_against_oracle gated, bit for bit, after the refused call


# ------------------------------------------------------------------------------------------------ 9. module and loop (GPU)
@pytest.mark.gpu
def test_module_forward_shared_fills_every_grad_like_the_engine_path():
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.engine import flat_from_state_dict
    s = _setup(**BASE)
    cfg = SimpleNamespace(**dict(vars(s.cfg), seed=5))
    model = VSLNet(cfg, np.zeros((cfg.word_size - 2, cfg.word_dim), np.float32))
    model.load_state_dict(s.P, strict=True)
    model = model.cuda()
    model.train()
    d = s.d
    h, sl, el = model.forward_shared(d['word_ids'], d['char_ids'], d['vfeats'], d['video_v_mask'], d['q_mask'], s.sb['idx'])
    loss = model.compute_loss(sl, el, d['s_labels'], d['e_labels']) + 5.0 * model.compute_highlight_loss(h, d['h_labels'], d['v_mask'])
    loss.backward()
    seed = (model._seed << 20) + model._step
    # the engine path on the same parameters and the same step seed
    eng = model._engine
    flat = flat_from_state_dict(eng, s.P)
    assert torch.equal(flat, model._flat)
    h2, sl2, el2 = eng.forward_shared(flat, s.pad, s.glove, d['word_ids'], d['char_ids'], d['vfeats'], d['video_v_mask'], d['q_mask'], s.sb['idx'], training=True, seed=seed)
    # the seeds as the module's two loss calls make them (compute_loss: weights 1, 0 on an all-ones mask; compute_highlight_loss: weights 0, 1; autograd
    # scales the highlight seed by the 5.0 of `loc + 5.0 * hl`): the same kernels on the same seeds, so the gradients are EQUAL, bit for bit
    B, T = sl2.shape
    zb, zh, ones = torch.zeros(B, dtype=torch.int64, device='cuda'), torch.zeros(B, T, dtype=torch.int64, device='cuda'), torch.ones(B, T, device='cuda')
    l_loc, _, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], zh, 1.0, 0.0, scores=sl2, start_logits=sl2, end_logits=el2, v_mask=ones)
    l_hl, d_h, _, _ = eng.loss(zb, zb, d['h_labels'], 0.0, 1.0, scores=h2, start_logits=h2, end_logits=h2, v_mask=d['v_mask'])
    g = eng.views(eng.backward(d_h * 5.0, d_sl, d_el, eng.new_flat()))
    torch.cuda.synchronize()
    assert torch.equal(sl.detach(), sl2) and torch.equal(el.detach(), el2) and torch.equal(h.detach(), h2)
    assert float(loss.detach()) == float(l_loc[0] + 5.0 * l_hl[1])
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None, n
        assert torch.equal(p.grad, g[n]), (n, float((p.grad - g[n]).abs().max()))
    model.eval()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='encode_video'):
            model.forward_shared(d['word_ids'], d['char_ids'], d['vfeats'], d['video_v_mask'], d['q_mask'], s.sb['idx'])


@pytest.mark.gpu
def test_main_trains_through_the_shared_step_and_tests_the_checkpoint(tmp_path):
    import main
    argv = ['--task', 'synthetic', '--predictor', 'transformer', '--epochs', '1', '--max_pos_len', '32', '--video_feature_dim', '64', '--synthetic_train', '64',
            '--synthetic_test', '16', '--batch_size', '16', '--period', '1', '--model_dir', str(tmp_path / 'ckpt'), '--share_videos']
    lines = []
    out = main.run(argv + ['--mode', 'train'], log=lambda *a: lines.append(' '.join(str(x) for x in a)))
    losses = [v for _, v in out['history'] if isinstance(v, float)]
    assert out['steps'] == 4 and len(losses) == 4 and all(np.isfinite(losses)), out['history']
    assert any(f.endswith('.t7') for f in os.listdir(out['model_dir']))
    with open(os.path.join(out['model_dir'], 'configs.json')) as f:
        assert json.load(f)['share_videos'] is True
    res = main.run(argv + ['--mode', 'test'], log=lambda *a: None)
    assert all(np.isfinite(res[k]) for k in ('r1i3', 'r1i5', 'r1i7', 'mIoU'))
    for extra, word in ((['--data', 'loader'], 'resident'), (['--optimizer', 'torch'], 'fused')):
        with pytest.raises(ValueError, match=word):
            main.run(argv + ['--mode', 'train'] + extra, log=lambda *a: None)
