"""num_heads 4 and 16 (head sizes 32 and 8): the attention core of kernels_attn_hd.hip (shared parts: attn.hpp; dispatch: kernels_attn.hip), through every layer above it.

CPU-only tests: vsl_create's head-count validation (it runs before the device query) and the oracle against fixtures the reference
itself produced with 4 and 16 heads (tools/make_golden_heads.py; each fixture is split into files under 1 MiB).
GPU tests: eval-mode parity with those fixtures and with the oracle over ragged lengths, both dropout hash families (L <= 256 element
hashes, L > 256 key pairs) and multi-slab dQ; training mode on the same dropout masks; finite differences; the data-parallel shard sum;
the autograd module and the CLI.  Gates are those of test_oracle_golden.py, test_hip_parity.py and test_hip_training.py."""
import ctypes
import glob
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import GOLDEN, ROOT, assert_forced_relu_inside_noise, check_training_against_oracle, grad_tol, load_golden

HEAD_CASES = ['heads4_tf', 'heads16_tf']


def load_heads_golden(name):
    cfg, P, b, z = load_golden(name)
    z = {k: z[k] for k in z.files}
    for part in sorted(glob.glob(os.path.join(GOLDEN, name + '.part*.npz'))):
        zp = np.load(part, allow_pickle=False)
        z.update({k: zp[k] for k in zp.files})
    return cfg, P, b, z


# ------------------------------------------------------------------------------------------------ vsl_create (no GPU)
def _create(num_heads):
    from vslnet_amd import build
    from vslnet_amd.engine import vsl_config
    lib = ctypes.CDLL(build.build())
    lib.vsl_last_error.restype = ctypes.c_char_p
    cfg = vsl_config(128, num_heads, 32, 64, 300, 50, 52, 40, 1, 0.0, 0)
    h = ctypes.c_void_p()
    rc = lib.vsl_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = lib.vsl_last_error().decode()
    if rc == 0:
        lib.vsl_destroy(h)
    return rc, msg


@pytest.mark.parametrize('num_heads', [4, 16])
def test_create_accepts_4_and_16_heads(num_heads):
    rc, msg = _create(num_heads)
    if torch.cuda.is_available():
        assert rc == 0, msg
    else:
        assert rc != 0 and 'no HIP device' in msg, msg          # the only refusal left on a machine without a GPU


def test_create_still_refuses_other_head_counts():
    rc, msg = _create(32)
    assert rc != 0 and 'num_heads=32' in msg and '4, 8 and 16' in msg, msg
    rc, msg = _create(7)
    assert rc != 0 and 'not a multiple of attention heads' in msg, msg


# ------------------------------------------------------------------------------------------------ oracle vs reference (no GPU)
def _close(a, b, atol=2e-5, what=''):
    a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
    finite = np.abs(b) < 1e29
    assert np.array_equal(a[~finite], b[~finite]), what + ': masked entries must be exactly -1e30'
    err = np.abs(a[finite] - b[finite]).max() if finite.any() else 0.0
    atol = atol * max(1.0, float(np.abs(b[finite]).max()) if finite.any() else 1.0)
    assert err <= atol, '%s: max abs err %.3e > %.1e' % (what, err, atol)


@pytest.mark.parametrize('name', HEAD_CASES)
def test_oracle_reproduces_the_reference_at_other_head_counts(name):
    cfg, P, b, z = load_heads_golden(name)
    assert cfg.num_heads == {'heads4_tf': 4, 'heads16_tf': 16}[name]
    want = {}
    with torch.no_grad():
        h, sl, el = O.forward(P, cfg, b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'], training=False, want=want)
    for key, tap in [('video_affine', 'video_affine.0'), ('embedding_net', 'embedding_net.0'), ('venc', 'feature_encoder.0'),
                     ('qenc', 'feature_encoder.1'), ('cq_attention', 'cq_attention.0'), ('cq_concat', 'cq_concat.0')]:
        _close(want[key], z['tap.' + tap], what=key)
    _close(want['pred_parts']['pred_s'], z['tap.pred_encoder.0'], what='pred enc 1')
    _close(want['pred_parts']['pred_e'], z['tap.pred_encoder.1'], what='pred enc 2')
    _close(h, z['out.h_score'], atol=5e-6, what='h_score')
    _close(sl, z['out.start_logits'], what='start_logits')
    _close(el, z['out.end_logits'], what='end_logits')
    _close(O.highlight_loss(h, b['h_labels'], b['v_mask']), z['out.highlight_loss'], atol=1e-5, what='hl loss')
    _close(O.span_loss(sl, el, b['s_labels'], b['e_labels']), z['out.loc_loss'], atol=2e-5, what='loc loss')
    Pg = {k: v.clone().requires_grad_(k not in O.FROZEN) for k, v in P.items()}
    total, _ = O.total_loss(Pg, cfg, b, training=False)
    total.backward()
    n = 0
    for k in z:
        if k.startswith('grad.'):
            g = Pg[k[5:]].grad
            g = torch.zeros_like(Pg[k[5:]]) if g is None else g
            err = float(np.abs(g.numpy() - z[k]).max())
            assert err <= grad_tol(z[k]), '%s: grad err %.3e (tol %.3e)' % (k, err, grad_tol(z[k]))
            n += 1
    assert n >= 40


# ------------------------------------------------------------------------------------------------ GPU
def _engine(cfg, P):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    eng = Engine(cfg)
    return eng, flat_from_state_dict(eng, P)


def _dev(b):
    return {k: v.cuda().contiguous() for k, v in b.items()}


def _fwd(eng, flat, P, d, training=False, seed=0, sample_offset=0):
    return eng.forward(flat, P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda(), d['word_ids'],
                       d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], training=training, seed=seed, sample_offset=sample_offset)


def _err(got, ref, atol):
    got = got.detach().float().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = ref.detach().float().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert got.shape == ref.shape
    big = np.abs(ref) > 1e29
    if not np.array_equal(got[big], ref[big]):
        return float('inf'), 0.0
    fin = ~big
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    return (err if np.isfinite(err) else float('inf')), atol * max(1.0, float(np.abs(ref[fin]).max()) if fin.any() else 1.0)


def _grads_vs_oracle(eng, flat, P, cfg, b, d, losses_atol=2e-5):
    """eval mode: engine loss + every parameter gradient against the oracle on the ReLU branches the GPU forward took"""
    from tests.helpers import relu_flips
    B, T = b['v_mask'].shape
    Lq = b['q_mask'].shape[1]
    h, sl, el = _fwd(eng, flat, P, d)
    losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
    g = eng.backward(d_h, d_sl, d_el, eng.new_flat())
    torch.cuda.synchronize()
    O.record_relu_signs()
    with torch.no_grad():
        O.forward(P, cfg, b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'])
    flips, hip_masks = relu_flips(eng, B, T, Lq, predictor=cfg.predictor)
    O.record_relu_signs(False)
    O.force_relu_signs(hip_masks)
    Pg = {k: v.clone().requires_grad_(k not in O.FROZEN) for k, v in P.items()}
    total, (oh, osl, oel, _, _) = O.total_loss(Pg, cfg, b, training=False)
    O.force_relu_signs(None)
    assert_forced_relu_inside_noise(O, flips)
    total.backward()
    bad = []
    for what, got, ref, atol in [('h_score', h, oh, 2e-5), ('start_logits', sl, osl, 1e-4), ('end_logits', el, oel, 1e-4)]:
        err, tol = _err(got, ref, atol)
        if not err <= tol:
            bad.append((what, err, tol))
    if not abs(float(losses[2]) - float(total.detach())) <= losses_atol * max(1.0, abs(float(total.detach()))):
        bad.append(('loss', float(losses[2]), float(total.detach())))
    for k, t in eng.views(g).items():
        ref = Pg[k].grad if Pg[k].grad is not None else torch.zeros_like(Pg[k])
        err, tol = float((t.cpu() - ref).abs().max()), 1e-4 * float(ref.abs().max()) + 1e-6
        if not err <= tol:
            bad.append((k, err, tol))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize('name', HEAD_CASES)
def test_eval_forward_and_gradients_match_the_reference(name):
    from tests.helpers import relu_flips
    cfg, P, b, z = load_heads_golden(name)
    d = _dev(b)
    eng, flat = _engine(cfg, P)
    h, sl, el = _fwd(eng, flat, P, d)
    losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
    g = eng.backward(d_h, d_sl, d_el, eng.new_flat())
    torch.cuda.synchronize()
    B, T = b['v_mask'].shape
    Lq = b['q_mask'].shape[1]
    bad = []
    for what, view, tap, atol in [('video_affine', (B, T), 'video_affine.0', 1e-4), ('embedding_net', (B, Lq), 'embedding_net.0', 1e-4),
                                  ('venc', (B, T), 'feature_encoder.0', 1e-4), ('qenc', (B, Lq), 'feature_encoder.1', 1e-4),
                                  ('cq_attention', (B, T), 'cq_attention.0', 1e-4), ('cq_concat', (B, T), 'cq_concat.0', 1e-4),
                                  ('pred_s', (B, T), 'pred_encoder.0', 1e-4), ('pred_e', (B, T), 'pred_encoder.1', 1e-4)]:
        err, tol = _err(eng.ws_view(what, view + (128,)), z['tap.' + tap], atol)
        if not err <= tol:
            bad.append((what, err, tol))
    for what, got, key, atol in [('h_score', h, 'out.h_score', 2e-5), ('start_logits', sl, 'out.start_logits', 1e-4),
                                 ('end_logits', el, 'out.end_logits', 1e-4), ('loc_loss', losses[0], 'out.loc_loss', 2e-5),
                                 ('highlight_loss', losses[1], 'out.highlight_loss', 2e-5)]:
        err, tol = _err(got, z[key], atol)
        if not err <= tol:
            bad.append((what, err, tol))
    # the gradients are comparable with the reference's only where both forwards took the same ReLU branches (test_hip_parity.py)
    O.record_relu_signs()
    with torch.no_grad():
        O.forward(P, cfg, b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'])
    flips, _ = relu_flips(eng, B, T, Lq)
    O.record_relu_signs(False)
    if flips == 0:
        for k, t in eng.views(g).items():
            if 'grad.' + k in z:
                err, tol = float(np.abs(t.cpu().numpy() - z['grad.' + k]).max()), grad_tol(z['grad.' + k])
                if not err <= tol:
                    bad.append((k, err, tol))
    assert not bad, (flips, bad[:6])
    bad = _grads_vs_oracle(eng, flat, P, cfg, b, d)
    assert not bad, bad[:6]


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [4, 16])
@pytest.mark.parametrize('T,Lq,predictor', [(37, 7, 'transformer'), (128, 40, 'transformer'), (200, 7, 'rnn'), (301, 40, 'transformer'),
                                            (301, 7, 'rnn')])
def test_eval_mode_matches_oracle(num_heads, T, Lq, predictor):
    """ragged lengths; L <= 128, 128 < L <= 256 and L > 256 (two dQ slabs) on the video side, Lq = 7 / 40 on the query side"""
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=max(T, Lq), word_size=52, predictor=predictor, num_heads=num_heads)
    P = O.random_params(cfg, seed=31)
    b = O.synthetic_batch(cfg, 3 if T < 256 else 2, T, Lq, 6, seed=32, ragged=True)
    eng, flat = _engine(cfg, P)
    bad = _grads_vs_oracle(eng, flat, P, cfg, b, _dev(b))
    assert not bad, bad[:6]


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [4, 16])
@pytest.mark.parametrize('B,T,Lq,predictor', [(3, 40, 7, 'transformer'), (2, 128, 20, 'transformer'), (2, 200, 9, 'transformer'),
                                              (2, 301, 7, 'transformer'), (4, 33, 6, 'rnn')])
def test_training_mode_matches_oracle_on_the_same_dropout_masks(num_heads, B, T, Lq, predictor):
    check_training_against_oracle(B, T, Lq, 6, cfg=dict(video_feature_dim=64, predictor=predictor, num_heads=num_heads), param_seed=21, batch_seed=22,
                                  step_seed=(7 << 33) + 12345)


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [4, 16])
@pytest.mark.parametrize('T', [48, 160])
def test_dropout_forward_backward_consistency_by_finite_differences(num_heads, T):
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=T, word_size=52, drop_rate=0.2, num_heads=num_heads)
    P = O.random_params(cfg, seed=3)
    d = _dev(O.synthetic_batch(cfg, B=4, T=T, Lq=9, Lc=7, seed=4, ragged=True))
    eng, flat = _engine(cfg, P)
    seed = 1234567

    def loss(fl):
        _fwd(eng, fl, P, d, True, seed)
        losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
        return float(losses[2].item()), (d_h, d_sl, d_el)
    f0, seeds = loss(flat)
    g = eng.backward(*seeds, eng.new_flat()).clone()
    assert loss(flat)[0] == f0, 'training-mode forward is not deterministic for a fixed seed'
    gd = g.double()
    assert np.isfinite(float(gd.norm())) and float(gd.norm()) > 0
    rs = np.random.RandomState(0)
    for trial in range(3):
        v = gd if trial == 0 else gd * torch.from_numpy(rs.choice([0.0, 1.0], size=gd.numel())).cuda()
        v = v / float(v.norm())
        pred = float((gd * v).sum())
        eps = 0.02 / max(abs(pred), 1e-3)
        fp, _ = loss((flat.double() + eps * v).float())
        fm, _ = loss((flat.double() - eps * v).float())
        fd = (fp - fm) / (2 * eps)
        assert abs(fd - pred) <= 0.03 * abs(pred) + 2e-3, 'trial %d: finite difference %.6f vs g.v %.6f' % (trial, fd, pred)


@pytest.mark.gpu
def test_data_parallel_shards_add_up_at_4_heads():
    """training mode, global normalisers and sample_offset: three uneven shards reproduce the full batch's gradient (and the backward
    is deterministic: two full-batch runs are bit-identical)"""
    from tests.helpers import hip_relu_masks
    B, T, Lq, Lc = 16, 128, 20, 10
    cfg = O.make_cfg(video_feature_dim=256, max_pos_len=T, word_size=1002, drop_rate=0.2, num_heads=4)
    P = O.random_params(cfg, seed=12345)
    b = O.synthetic_batch(cfg, B, T, Lq, Lc, seed=0, ragged=True)
    d = _dev(b)
    eng, flat = _engine(cfg, P)
    seed, msum = 20260928, float(b['v_mask'].sum())

    def grads_of(lo, hi):
        dd = {k: v[lo:hi].contiguous() for k, v in d.items()}
        _fwd(eng, flat, P, dd, True, seed, sample_offset=lo)
        _, dh, dsl, del_ = eng.loss(dd['s_labels'], dd['e_labels'], dd['h_labels'], 1.0, 5.0, inv_batch=1.0 / B, mask_sum=msum)
        out = eng.backward(dh, dsl, del_, eng.new_flat()).double().clone()
        torch.cuda.synchronize()
        return out, hip_relu_masks(eng, hi - lo, T, Lq)
    full, fm = grads_of(0, B)
    full2, _ = grads_of(0, B)
    assert torch.equal(full, full2)
    parts = torch.zeros_like(full)
    moved = 0
    for lo, hi in [(0, 6), (6, 10), (10, B)]:
        g, m = grads_of(lo, hi)
        parts += g
        moved += sum(int((a != f[lo:hi]).sum()) for a, f in zip(m, fm))
    assert moved == 0, moved
    for k, t in eng.views(full).items():
        err = float((t - eng.views(parts)[k]).abs().max())
        assert err <= 2e-5 * float(t.abs().max()) + 1e-6, (k, err)


@pytest.mark.gpu
def test_module_with_4_heads_matches_the_engine():
    from vslnet_amd.model.VSLNet import VSLNet
    cfg, P, b, z = load_heads_golden('heads4_tf')
    m = VSLNet(cfg, np.zeros((cfg.word_size - 2, cfg.word_dim), np.float32))
    m.load_state_dict(P, strict=True)
    m = m.to('cuda').eval()
    d = _dev(b)
    h, sl, el = m(d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'])
    total = m.compute_loss(sl, el, d['s_labels'], d['e_labels']) + 5.0 * m.compute_highlight_loss(h, d['h_labels'], d['v_mask'])
    m.zero_grad()
    total.backward()
    eng, flat = _engine(cfg, P)
    eh, esl, eel = _fwd(eng, flat, P, d)
    losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
    g = eng.views(eng.backward(d_h, d_sl, d_el, eng.new_flat()))
    torch.cuda.synchronize()
    for got, ref in [(sl, esl), (el, eel), (h, eh)]:
        err, tol = _err(got, ref, 1e-5)
        assert err <= tol, (err, tol)
    assert abs(float(total.detach()) - float(losses[2])) <= 1e-5 * max(1.0, abs(float(total.detach())))
    bad = [n for n, p in m.named_parameters() if p.requires_grad and not torch.allclose(p.grad, g[n], rtol=0, atol=1e-6 + 1e-5 * float(g[n].abs().max()))]
    assert not bad, bad
    fin = np.abs(z['out.start_logits']) < 1e29
    assert np.abs(sl.detach().cpu().numpy() - z['out.start_logits'])[fin].max() < 1e-4 * max(1, np.abs(z['out.start_logits'][fin]).max())


@pytest.mark.gpu
def test_cli_trains_one_epoch_with_16_heads(tmp_path):
    argv = [sys.executable, os.path.join(ROOT, 'main.py'), '--task', 'synthetic', '--num_heads', '16', '--epochs', '1', '--max_pos_len', '32',
            '--video_feature_dim', '64', '--batch_size', '16', '--synthetic_train', '64', '--synthetic_test', '32', '--period', '1',
            '--model_dir', str(tmp_path)]
    r = subprocess.run(argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(line.rsplit('loss', 1)[1]) for line in r.stdout.splitlines() if '| loss' in line]
    assert len(losses) >= 4 and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
