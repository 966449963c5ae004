"""Gradients with respect to the video features: vsl_input_grads (k_vproj_dx), Engine.input_grads, and `video_features.grad` through VSLNet.

dX = dropmask * (d_video_affine @ W): the one product the backward stops short of.  d_video_affine is what vsl_backward leaves in the workspace, W
is video_affine.linear.conv1d.weight as (128, Dv) in the parameter bucket, dropmask is the multiplier VisualProjection's dropout applied in the
forward (site 64, the oracle's dropout call 0).

CPU: the ABI (the export, version 9, vsl_io unmoved).
GPU, at the smallest shapes that reach every guard of the kernel -- B 3, T 37 (R = 111: three whole 32-row tiles and 15 rows), Lq 4, Lc 5, Dv 20 (below
one 32-column tile), 64 (below one 128-column block), 500 (off 32 and 128; two blocks per workgroup, the second ragged) and 1024 (several blocks,
four column phases):
  - the kernel alone against fp64 of its own inputs, at the Higham bound of a 128-term fp32 dot (130 u S per element: 128 for the chain in any
    order, one for the mask multiply, one to spare), with the exact-zero pattern of the mask;
  - against the oracle's autograd on the HIP path's dropout masks and ReLU branches, padded clips included, at the project's gradient gate;
  - through autograd (an nn.Linear adapter in front of the module), the shared step, sample_offset, accumulation, bf16 features;
  - nothing else of the step moves; every refusal by name."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import (ROOT, assert_forced_relu_inside_noise, check_training_against_oracle, grad_tol, hip_dropout, hip_relu_masks)
from tests.test_shared_train import hip_relu_masks_shared, replicated, shared_batch

SIZEOF_VSL_IO = 208             # ABI 9, `inference` last: the struct must not move
STEP_SEED = (7 << 33) + 12345   # (exercises the high word of the 64-bit seed too)
B, T, LQ, LC = 3, 37, 4, 5
WEIGHT = 'video_affine.linear.conv1d.weight'
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 1. the ABI (CPU)
def test_library_exports_vsl_input_grads_and_keeps_abi_9():
    from vslnet_amd import build, engine
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, 'vsl_input_grads')
    assert 'vsl_input_grads' in engine.ABI_SYMBOLS
    assert lib.vsl_abi_version() == 9 == engine.ABI_VERSION
    header = open(os.path.join(ROOT, 'include', 'vslnet_hip.h')).read()
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', header)
    assert re.search(r'\bint\s+vsl_input_grads\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    assert ctypes.sizeof(engine.vsl_io) == SIZEOF_VSL_IO


# ------------------------------------------------------------------------------------------------ helpers (GPU)
def _setup(Dv, n=B, drop_rate=0.2, predictor='transformer', param_seed=21, batch_seed=22):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg = O.make_cfg(video_feature_dim=Dv, max_pos_len=max(T, LQ), word_size=102, drop_rate=drop_rate, predictor=predictor)
    P = O.random_params(cfg, seed=param_seed)
    b = O.synthetic_batch(cfg, n, T, LQ, LC, seed=batch_seed, ragged=True)
    d = {k: v.cuda().contiguous() for k, v in b.items()}
    eng = Engine(cfg)
    return SimpleNamespace(cfg=cfg, P=P, b=b, d=d, eng=eng, flat=flat_from_state_dict(eng, P), pad=P['embedding_net.word_emb.pad_vec'].cuda(),
                           glove=P['embedding_net.word_emb.glove_vec'].cuda(), n=n, Dv=Dv, msum=float(b['v_mask'].sum()))


def _step(s, training=True, seed=STEP_SEED, lo=0, hi=None, grads=None, vfeats=None, **kw):
    """forward + loss + backward of rows [lo, hi) of the batch as a shard of it (global normalisers, sample_offset = lo) -> (logits, flat gradient)"""
    hi = s.n if hi is None else hi
    dd = {k: v[lo:hi].contiguous() for k, v in s.d.items()}
    h, sl, el = s.eng.forward(s.flat, s.pad, s.glove, dd['word_ids'], dd['char_ids'], dd['vfeats'] if vfeats is None else vfeats[lo:hi].contiguous(),
                              dd['v_mask'], dd['q_mask'], training=training, seed=seed, sample_offset=lo)
    _, d_h, d_sl, d_el = s.eng.loss(dd['s_labels'], dd['e_labels'], dd['h_labels'], 1.0, 5.0, inv_batch=1.0 / s.n, mask_sum=s.msum)
    g = s.eng.backward(d_h, d_sl, d_el, s.eng.new_flat() if grads is None else grads, **kw)
    return sl, g


def assert_kernel_bound(eng, flat, dX, m, context):
    """dX (n, T, Dv) of the engine's last step against fp64 of the kernel's own inputs: |dX - m (G W)| <= 130 u m sum_j |G_rj W_jc| + 1e-30 per
    element, exactly 0 where the mask is 0 and nowhere else that the reference is not.  m: the mask as (n, T, Dv), or None = all ones."""
    n, t, Dv = dX.shape
    torch.cuda.synchronize()
    G = eng.ws_view('d_video_affine', (n * t, 128)).cpu().double()
    W = eng.views(flat)[WEIGHT].reshape(128, Dv).cpu().double()
    m = (torch.ones(n * t, Dv) if m is None else m.reshape(n * t, Dv)).double()
    got = dX.reshape(n * t, Dv).cpu().double()
    ref, S = m * (G @ W), m * (G.abs() @ W.abs())
    err, bound = (got - ref).abs(), 130.0 * U * S + 1e-30
    print('[input-grads] %s: |dX|inf %.3e, max err %.3e, worst element at %.4f of its bound' % (context, float(got.abs().max()), float(err.max()),
                                                                                             float((err / bound).max())))
    assert float(ref.abs().max()) > 0.0, context
    assert bool((err <= bound).all()), (context, float((err / bound).max()))
    zero = got == 0
    assert bool(zero[m == 0].all()), context
    assert not bool(zero[(m != 0) & (ref != 0)].any()), context


def site_vis_mask(seed, shape, p):
    """VisualProjection's dropout multiplier: the oracle's dropout call 0 = SITE_VIS, keyed by the row-major element index of `shape`"""
    return hip_dropout(seed)(0, tuple(shape), p)


# ------------------------------------------------------------------------------------------------ 2. the kernel alone against fp64 (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize('Dv', [20, 64, 500, 1024])
def test_kernel_meets_the_fp32_dot_bound_and_the_masks_zero_pattern(Dv):
    s = _setup(Dv)
    _step(s, training=True)
    dX = s.eng.input_grads()
    assert dX.shape == (B, T, Dv) and dX.dtype == torch.float32
    m = site_vis_mask(STEP_SEED, (B, T, Dv), s.cfg.drop_rate)
    assert 0.1 < float((m == 0).double().mean()) < 0.3
    assert_kernel_bound(s.eng, s.flat, dX, m, 'Dv %d train' % Dv)
    _step(s, training=False)
    assert_kernel_bound(s.eng, s.flat, s.eng.input_grads(), None, 'Dv %d eval' % Dv)


# ------------------------------------------------------------------------------------------------ 3. against the oracle (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize('shape,cfg', [((3, 37, 4, 5), dict(video_feature_dim=500)), ((2, 64, 9, 6), dict(video_feature_dim=1024, predictor='rnn'))],
                         ids=['B3-T37-Dv500', 'B2-T64-Dv1024-rnn'])
def test_input_gradient_matches_the_oracle_on_the_same_masks(shape, cfg):
    ns = check_training_against_oracle(*shape, cfg=cfg, step_seed=STEP_SEED, context='input grads')
    dX = ns.eng.input_grads().cpu()
    try:
        O.force_relu_signs(ns.hip_masks)
        O.force_dropout(hip_dropout(STEP_SEED))
        b = dict(ns.b)
        b['vfeats'] = ns.b['vfeats'].clone().requires_grad_()
        total, _ = O.total_loss(ns.P, ns.cfg, b, training=True)
        O.force_relu_signs(None)
        O.force_dropout(None)
        assert_forced_relu_inside_noise(O, 'input grads')
        total.backward()
    finally:
        O.force_relu_signs(None)
        O.force_dropout(None)
    ref = b['vfeats'].grad
    assert ref.shape == dX.shape
    err, tol = float((dX - ref).abs().max()), grad_tol(ref.numpy())
    pad = ns.b['v_mask'] == 0
    print('[input-grads] oracle %s: |g|inf %.3e (padded clips %.3e), err %.3e = %.4f of the gate' % (shape, float(ref.abs().max()), float(ref[pad].abs().max()),
                                                                                                 err, err / tol))
    assert bool(pad.any()) and float(ref[pad].abs().max()) > 0.0            # padded clips get a gradient: they are part of the contract
    assert err <= tol, (err, tol)


# ------------------------------------------------------------------------------------------------ 4. through autograd (GPU)
@pytest.mark.gpu
def test_an_adapter_in_front_of_the_module_gets_its_gradient():
    from vslnet_amd.model.VSLNet import VSLNet
    Dv = 500
    s = _setup(Dv)
    cfg = SimpleNamespace(**dict(vars(s.cfg), seed=5))
    model = VSLNet(cfg, np.zeros((cfg.word_size - 2, cfg.word_dim), np.float32))
    model.load_state_dict(s.P, strict=True)
    model = model.cuda().eval()                     # eval: the oracle needs no dropout masks (grad is enabled: the saved path)
    torch.manual_seed(3)
    adapter = torch.nn.Linear(24, Dv)
    x = torch.randn(B, T, 24) * s.b['v_mask'][:, :, None]
    Wa, ba = adapter.weight.detach().clone(), adapter.bias.detach().clone()
    adapter = adapter.cuda()
    d = s.d

    def run(feats):
        model.zero_grad(set_to_none=True)
        h, sl, el = model(d['word_ids'], d['char_ids'], feats, d['v_mask'], d['q_mask'])
        loss = model.compute_loss(sl, el, d['s_labels'], d['e_labels']) + 5.0 * model.compute_highlight_loss(h, d['h_labels'], d['v_mask'])
        loss.backward()
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}
    feats = adapter(x.cuda())
    feats.retain_grad()
    g_with = run(feats)
    assert feats.grad is not None and feats.grad.shape == (B, T, Dv) and feats.grad.dtype == feats.dtype
    assert adapter.weight.grad is not None and adapter.bias.grad is not None
    masks = hip_relu_masks(model._engine, B, T, LQ)
    g_without = run(feats.detach())
    for n in g_with:                                # asking for the input gradient moves no parameter gradient
        assert torch.equal(g_with[n], g_without[n]), n
    # the oracle's composite gradient: the adapter, then the model, on the HIP forward's ReLU branches
    Wr, br = Wa.clone().requires_grad_(), ba.clone().requires_grad_()
    b = dict(s.b)
    b['vfeats'] = x @ Wr.t() + br
    try:
        O.force_relu_signs(masks)
        total, _ = O.total_loss(s.P, s.cfg, b, training=False)
        O.force_relu_signs(None)
        assert_forced_relu_inside_noise(O, 'adapter')
        total.backward()
    finally:
        O.force_relu_signs(None)
    for got, ref, nm in ((adapter.weight.grad, Wr.grad, 'weight'), (adapter.bias.grad, br.grad, 'bias')):
        err, tol = float((got.cpu() - ref).abs().max()), grad_tol(ref.numpy())
        print('[input-grads] adapter %s: |g|inf %.3e, err %.3e = %.4f of the gate' % (nm, float(ref.abs().max()), err, err / tol))
        assert err <= tol, (nm, err, tol)


# ------------------------------------------------------------------------------------------------ 5. the shared step (GPU)
def _shared_setup(Dv, drop_rate):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    N, idx = 2, [0, 1, 1, 0, 1]
    cfg = O.make_cfg(video_feature_dim=Dv, max_pos_len=max(T, LQ), word_size=102, drop_rate=drop_rate)
    P = O.random_params(cfg, seed=21)
    sb = shared_batch(cfg, N, idx, T, LQ, LC, seed=22)
    d = {k: v.cuda().contiguous() for k, v in sb.items() if torch.is_tensor(v)}
    eng = Engine(cfg)
    flat = flat_from_state_dict(eng, P)
    eng.forward_shared(flat, P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda(), d['word_ids'], d['char_ids'],
                       d['vfeats'], d['video_v_mask'], d['q_mask'], idx, training=True, seed=STEP_SEED)
    _, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
    eng.backward(d_h, d_sl, d_el, eng.new_flat())
    return SimpleNamespace(cfg=cfg, P=P, sb=sb, eng=eng, flat=flat, N=N, idx=idx, Dv=Dv)


@pytest.mark.gpu
def test_shared_step_gives_each_videos_gradient_summed_over_its_queries():
    s = _shared_setup(500, 0.0)
    dX = s.eng.input_grads()
    assert dX.shape == (s.N, T, s.Dv)
    assert_kernel_bound(s.eng, s.flat, dX, None, 'shared, drop 0')
    masks = hip_relu_masks_shared(s.eng, s.N, len(s.idx), T, LQ, 'transformer')
    masks[:4] = [m[s.idx] for m in masks[:4]]       # the video pass' branches, per query of the replicated batch
    b = replicated(s.sb)
    b['vfeats'] = b['vfeats'].clone().requires_grad_()
    try:
        O.force_relu_signs(masks)
        total, _ = O.total_loss(s.P, s.cfg, b, training=True)
        O.force_relu_signs(None)
        assert_forced_relu_inside_noise(O, 'shared')
        total.backward()
    finally:
        O.force_relu_signs(None)
    ref = torch.zeros(s.N, T, s.Dv).index_add_(0, torch.as_tensor(s.idx), b['vfeats'].grad)
    err, tol = float((dX.cpu() - ref).abs().max()), grad_tol(ref.numpy())
    print('[input-grads] shared: |g|inf %.3e, err %.3e = %.4f of the gate' % (float(ref.abs().max()), err, err / tol))
    assert err <= tol, (err, tol)


@pytest.mark.gpu
def test_shared_step_keys_the_mask_by_the_video_tensor():
    s = _shared_setup(500, 0.2)
    assert_kernel_bound(s.eng, s.flat, s.eng.input_grads(), site_vis_mask(STEP_SEED, (s.N, T, s.Dv), 0.2), 'shared, drop 0.2')


# ------------------------------------------------------------------------------------------------ 6. other modes (GPU)
@pytest.mark.gpu
def test_a_shard_continues_the_full_batchs_mask_and_accumulation_gives_the_micro_batchs_rows():
    Dv, n = 500, 5
    s = _setup(Dv, n=n)
    m = site_vis_mask(STEP_SEED, (n, T, Dv), s.cfg.drop_rate)
    _step(s)
    full = s.eng.input_grads()
    assert_kernel_bound(s.eng, s.flat, full, m, 'full batch')
    _step(s, lo=2)                                  # rows 2.. as a shard: B 3, sample_offset 2
    shard = s.eng.input_grads()
    assert shard.shape == (B, T, Dv)
    assert_kernel_bound(s.eng, s.flat, shard, m[2:], 'shard at sample_offset 2')
    assert torch.equal(shard == 0, full[2:] == 0)
    # one optimizer step over two micro-batches: each call gives its own micro-batch's rows
    bucket = s.eng.new_flat()
    _step(s, lo=0, hi=2, grads=bucket)
    assert_kernel_bound(s.eng, s.flat, s.eng.input_grads(), m[:2], 'micro-batch 0')
    _step(s, lo=2, grads=bucket, accumulate=True)
    acc = s.eng.input_grads()
    assert_kernel_bound(s.eng, s.flat, acc, m[2:], 'micro-batch 1, accumulate')
    assert torch.equal(acc, shard)                  # (the same shard of the same step: the same bits)


@pytest.mark.gpu
def test_bf16_features_get_the_fp32_gradient():
    Dv = 1024
    s = _setup(Dv)
    _step(s, vfeats=s.d['vfeats'].to(torch.bfloat16))
    dX = s.eng.input_grads()
    assert dX.dtype == torch.float32
    assert_kernel_bound(s.eng, s.flat, dX, site_vis_mask(STEP_SEED, (B, T, Dv), s.cfg.drop_rate), 'bf16 features')


# ------------------------------------------------------------------------------------------------ 7. nothing else moves (GPU)
@pytest.mark.gpu
def test_the_call_is_one_launch_that_changes_nothing_else():
    s = _setup(500)
    eng = s.eng
    runs = []
    for ask in (False, True):
        eng.profile_select('*')
        try:
            _, g = _step(s, seed=STEP_SEED)
            torch.cuda.synchronize()
            names = [r['name'] for r in eng.profile_launches()]
            assert 'vproj_dx' not in names, names                   # the step itself launches nothing for the feature
            dx = None
            if ask:
                dx = (eng.input_grads().clone(), eng.input_grads().clone())
                torch.cuda.synchronize()
                after = [r['name'] for r in eng.profile_launches()]
                assert after[:len(names)] == names and after[len(names):] == ['vproj_dx', 'vproj_dx'], after[len(names):]
        finally:
            eng.profile_select(None)
        g = g.clone()
        sl, _ = _step(s, seed=STEP_SEED + 1)
        torch.cuda.synchronize()
        runs.append((g, sl.clone(), dx))
    assert torch.equal(runs[0][0], runs[1][0])                      # the flat gradient
    assert torch.equal(runs[0][1], runs[1][1])                      # the next step's logits
    assert torch.equal(*runs[1][2])                                 # two calls: identical bits


# ------------------------------------------------------------------------------------------------ 8. misuse (GPU)
@pytest.mark.gpu
def test_misuse_fails_by_name_and_leaves_the_engine_usable():
    import ctypes as C
    from vslnet_amd.dp import FlatAdamW
    from vslnet_amd.engine import VslError, vsl_shared_io, _ptr
    Dv = 64
    s = _setup(Dv)
    eng, d = s.eng, s.d
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(B, T, Dv, device='cuda')

    def raw(io, sh, dst):
        eng._call(eng.lib.vsl_input_grads(eng.h, C.byref(io), None if sh is None else C.byref(sh), _ptr(dst), stream))
    with pytest.raises(VslError, match='no forward'):
        eng.input_grads()
    # a forward without a backward
    eng.forward(s.flat, s.pad, s.glove, d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], training=True, seed=STEP_SEED)
    with pytest.raises(VslError, match='vsl_input_grads: no backward has run since'):
        eng.input_grads()
    _step(s)
    io = eng._last
    # NULL output
    with pytest.raises(VslError, match='vsl_input_grads: d_video_features is NULL'):
        raw(io, None, None)
    # an sh after an ordinary forward
    sh = vsl_shared_io()
    idx = torch.zeros(B, dtype=torch.int32, device='cuda')
    sh.N, sh.video_index, sh.video_v_mask = B, _ptr(idx), _ptr(d['v_mask'])
    with pytest.raises(VslError, match='vsl_input_grads: the handle\'s last forward was not vsl_forward_shared'):
        raw(io, sh, out)
    # the refusals touched nothing: the call still works, with the bound
    m = site_vis_mask(STEP_SEED, (B, T, Dv), s.cfg.drop_rate)
    assert_kernel_bound(eng, s.flat, eng.input_grads(out=out), m, 'after refusals')
    # a backward that stepped the parameters: refused; backward, input_grads, adamw_step is the order that gives both
    flat = s.flat.clone()
    opt = FlatAdamW(flat, eng.layout, lr=1e-3, num_train_steps=10, clip_norm=0.05, engine=eng)
    keep, s.flat = s.flat, flat
    try:
        _step(s, fused_step=opt.fused_step())
        assert not torch.equal(flat, keep)
        with pytest.raises(VslError, match='vsl_input_grads: the last backward applied fused_step'):
            eng.input_grads()
    finally:
        s.flat = keep
    _, g = _step(s)
    dX = eng.input_grads()
    mom, var = torch.zeros_like(s.flat), torch.zeros_like(s.flat)
    stepped = s.flat.clone()
    eng.adamw_step(stepped, g, mom, var, 1e-3, 1, clip_norm=0.05, norm_from_backward=True)
    assert_kernel_bound(eng, s.flat, dX, m, 'backward, input_grads, then adamw_step')
    # forwards that saved nothing
    eng.forward(s.flat, s.pad, s.glove, d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], inference=True)
    with pytest.raises(VslError, match='saved nothing'):
        eng.input_grads()
    with pytest.raises(VslError, match='vsl_input_grads: the last forward saved nothing'):
        raw(eng._last, None, out)
    enc = eng.encode_video(s.flat, d['vfeats'], d['v_mask'])
    with pytest.raises(VslError, match='saved nothing'):
        eng.input_grads()
    with pytest.raises(VslError, match='vsl_input_grads: (the last forward saved nothing|no backward has run since)'):
        raw(io, None, out)                          # (the io of the earlier training step: its saves are gone)
    eng.localize(s.flat, s.pad, s.glove, enc, [0, 1, 2], d['word_ids'], d['char_ids'], d['q_mask'])
    with pytest.raises(VslError, match='saved nothing'):
        eng.input_grads()
    # a shared step: sh = NULL and another N are refused with vsl_backward's / vsl_backward_shared's messages
    vidx = [0, 1, 1]
    eng.forward_shared(s.flat, s.pad, s.glove, d['word_ids'], d['char_ids'], d['vfeats'][:2].contiguous(), d['v_mask'][:2].contiguous(), d['q_mask'], vidx,
                       training=True, seed=STEP_SEED)
    lab = {k: d[k] for k in ('s_labels', 'e_labels')}
    v_mask_q = d['v_mask'][:2][torch.as_tensor(vidx).cuda()]
    h_labels = (d['h_labels'].float() * v_mask_q).long()
    _, d_h, d_sl, d_el = eng.loss(torch.zeros_like(lab['s_labels']), torch.zeros_like(lab['e_labels']), h_labels, 1.0, 5.0)
    eng.backward(d_h, d_sl, d_el, eng.new_flat())
    with pytest.raises(VslError, match='vsl_input_grads: the handle\'s last forward was vsl_forward_shared'):
        raw(eng._last, None, out)
    bad = vsl_shared_io()
    C.memmove(C.byref(bad), C.byref(eng._last_shared), C.sizeof(vsl_shared_io))
    bad.N = 3
    with pytest.raises(VslError, match='vsl_input_grads: N=3, but the last vsl_forward_shared ran over N=2 videos'):
        raw(eng._last, bad, out)
    assert_kernel_bound(eng, s.flat, eng.input_grads(), site_vis_mask(STEP_SEED, (2, T, Dv), s.cfg.drop_rate), 'shared step after refusals')
    # ... and an ordinary step still passes
    _step(s)
    assert_kernel_bound(eng, s.flat, eng.input_grads(), m, 'a following step')
