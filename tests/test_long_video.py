"""Long videos: 1024 < T <= 4096 clips (k_attn_dq of kernels_attn.hip: the attention backward's dQ query-major, one dQ slab).

CPU-only: validate_dataset refuses a record with more clips than the engine serves.
GPU: eval-mode parity with the oracle (both predictors, 4 / 8 / 16 heads, ragged lengths), training mode on the same dropout masks (the
key-pair hashes of L > 256), finite differences through the new dQ path, the data-parallel shard sum, determinism, an O(T) workspace, the
T > 4096 refusal, the autograd module, and the slab path behind VSL_ATTN_DQ_SLABS=1.  Gates are those of test_attention_heads.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import ROOT, check_training_against_oracle
from tests.test_attention_heads import _dev, _engine, _err, _fwd, _grads_vs_oracle


# ------------------------------------------------------------------------------------------------ no GPU
def _dataset(v_len):
    rec = {'sample_id': 7, 'vid': 'long_video', 'v_len': v_len, 's_ind': 0, 'e_ind': 3, 'w_ids': [2, 3], 'c_ids': [[1, 2], [3]]}
    return {'n_words': 10, 'n_chars': 10, 'train_set': [rec], 'val_set': None, 'test_set': []}


def test_validate_dataset_rejects_videos_longer_than_4096_clips():
    from vslnet_amd.data import validate_dataset
    cfg = O.make_cfg(max_pos_len=8192)
    with pytest.raises(ValueError, match=r'train_set record 7 \(vid long_video\): 5000 clips'):
        validate_dataset(_dataset(5000), cfg)
    with pytest.raises(ValueError, match=r'4097 clips'):
        validate_dataset(_dataset(100), cfg, features={'long_video': np.zeros((4097, 4), np.float32)})
    validate_dataset(_dataset(4096), cfg)
    validate_dataset(_dataset(5000), O.make_cfg(max_pos_len=4096))      # sampled down to max_pos_len clips


# ------------------------------------------------------------------------------------------------ GPU
def _cfg(T, num_heads=8, predictor='transformer', drop_rate=0.0, Lq=9):
    return O.make_cfg(video_feature_dim=64, max_pos_len=max(T, Lq), word_size=52, predictor=predictor, num_heads=num_heads,
                      drop_rate=drop_rate)


@pytest.mark.gpu
@pytest.mark.parametrize('T,B,num_heads,predictor', [(1025, 2, 8, 'transformer'), (1500, 2, 8, 'transformer'), (2048, 1, 8, 'transformer'),
                                                     (4096, 1, 8, 'transformer'), (1025, 2, 8, 'rnn'), (1500, 2, 8, 'rnn'),
                                                     (2048, 1, 8, 'rnn'), (1500, 2, 4, 'transformer'), (1500, 2, 16, 'transformer'),
                                                     (2048, 1, 4, 'transformer'), (2048, 1, 16, 'transformer')])
def test_eval_mode_matches_oracle_on_long_videos(T, B, num_heads, predictor):
    cfg = _cfg(T, num_heads, predictor)
    P = O.random_params(cfg, seed=41)
    b = O.synthetic_batch(cfg, B, T, 9, 6, seed=42, ragged=True)
    eng, flat = _engine(cfg, P)
    bad = _grads_vs_oracle(eng, flat, P, cfg, b, _dev(b))
    assert not bad, bad[:6]


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [8, 4, 16])
@pytest.mark.parametrize('T,B', [(1100, 2), (2048, 1)])
def test_training_mode_matches_oracle_on_the_same_dropout_masks(num_heads, T, B):
    check_training_against_oracle(B, T, 7, 6, cfg=dict(video_feature_dim=64, num_heads=num_heads), param_seed=51, batch_seed=52,
                                  step_seed=(5 << 33) + 4321)


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [8, 16])
def test_dropout_forward_backward_consistency_by_finite_differences(num_heads):
    T = 1100
    cfg = _cfg(T, num_heads, drop_rate=0.2)
    P = O.random_params(cfg, seed=3)
    d = _dev(O.synthetic_batch(cfg, B=2, T=T, Lq=9, Lc=7, seed=4, ragged=True))
    eng, flat = _engine(cfg, P)
    seed = 7654321

    def loss(fl):
        _fwd(eng, fl, P, d, True, seed)
        losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
        return float(losses[2].item()), (d_h, d_sl, d_el)
    f0, seeds = loss(flat)
    g = eng.backward(*seeds, eng.new_flat()).clone()
    assert loss(flat)[0] == f0, 'training-mode forward is not deterministic for a fixed seed'
    gd = g.double()
    assert np.isfinite(float(gd.norm())) and float(gd.norm()) > 0
    # the attention's query projection reaches the loss only through dQ: its own direction checks the new kernel
    qw = [(o, k) for n, o, k, _ in eng.layout if n.endswith('attention_block.query.conv1d.weight')]
    assert qw
    only_q = torch.zeros_like(gd)
    for o, k in qw:
        only_q[o:o + k] = gd[o:o + k]
    rs = np.random.RandomState(0)
    for trial in range(3):
        v = gd if trial == 0 else only_q if trial == 1 else gd * torch.from_numpy(rs.choice([0.0, 1.0], size=gd.numel())).cuda()
        v = v / float(v.norm())
        pred = float((gd * v).sum())
        eps = 0.02 / max(abs(pred), 1e-3)
        fp, _ = loss((flat.double() + eps * v).float())
        fm, _ = loss((flat.double() - eps * v).float())
        fd = (fp - fm) / (2 * eps)
        assert abs(fd - pred) <= 0.03 * abs(pred) + 2e-3, 'trial %d: finite difference %.6f vs g.v %.6f' % (trial, fd, pred)


def _train_grads(eng, flat, P, d, lo, hi, B, seed, msum):
    dd = {k: v[lo:hi].contiguous() for k, v in d.items()}
    _fwd(eng, flat, P, dd, True, seed, sample_offset=lo)
    _, dh, dsl, del_ = eng.loss(dd['s_labels'], dd['e_labels'], dd['h_labels'], 1.0, 5.0, inv_batch=1.0 / B, mask_sum=msum)
    out = eng.backward(dh, dsl, del_, eng.new_flat()).double().clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
def test_data_parallel_shards_add_up_at_2048_clips():
    from tests.helpers import hip_relu_masks
    B, T, Lq = 2, 2048, 9
    cfg = _cfg(T, drop_rate=0.2, Lq=Lq)
    P = O.random_params(cfg, seed=61)
    b = O.synthetic_batch(cfg, B, T, Lq, 6, seed=62, ragged=True)
    d = _dev(b)
    eng, flat = _engine(cfg, P)
    seed, msum = 20261016, float(b['v_mask'].sum())
    full = _train_grads(eng, flat, P, d, 0, B, B, seed, msum)
    fm = hip_relu_masks(eng, B, T, Lq)
    parts = torch.zeros_like(full)
    moved = 0
    for lo, hi in [(0, 1), (1, 2)]:
        parts += _train_grads(eng, flat, P, d, lo, hi, B, seed, msum)
        moved += sum(int((a != f[lo:hi]).sum()) for a, f in zip(hip_relu_masks(eng, hi - lo, T, Lq), fm))
    assert moved == 0, moved
    for k, t in eng.views(full).items():
        err = float((t - eng.views(parts)[k]).abs().max())
        assert err <= 2e-5 * float(t.abs().max()) + 1e-6, (k, err)


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [8, 4])
def test_backward_is_bit_identical_across_runs(num_heads):
    B, T = 2, 1500
    cfg = _cfg(T, num_heads, drop_rate=0.2)
    P = O.random_params(cfg, seed=71)
    b = O.synthetic_batch(cfg, B, T, 9, 6, seed=72, ragged=True)
    d = _dev(b)
    eng, flat = _engine(cfg, P)
    msum = float(b['v_mask'].sum())
    g1 = _train_grads(eng, flat, P, d, 0, B, B, 99, msum)
    g2 = _train_grads(eng, flat, P, d, 0, B, B, 99, msum)
    assert torch.equal(g1, g2)


def _workspace_floats(eng, B, T, Lq=9, Lc=6):
    n = ctypes.c_int64()
    rc = eng.lib.vsl_workspace_floats(eng.h, B, T, Lq, Lc, ctypes.byref(n))
    return rc, n.value


@pytest.mark.gpu
@pytest.mark.parametrize('predictor', ['transformer', 'rnn'])
def test_workspace_grows_linearly_in_T(predictor):
    cfg = _cfg(4097, predictor=predictor)
    eng, _ = _engine(cfg, O.random_params(cfg, seed=1))
    rc2, w2 = _workspace_floats(eng, 1, 2048)
    rc4, w4 = _workspace_floats(eng, 1, 4096)
    assert rc2 == 0 and rc4 == 0
    assert w4 <= 2.1 * w2, (w2, w4)


@pytest.mark.gpu
def test_more_than_4096_clips_are_refused():
    cfg = _cfg(4097)
    eng, _ = _engine(cfg, O.random_params(cfg, seed=1))
    rc, _ = _workspace_floats(eng, 1, 4097)
    assert rc != 0
    msg = eng.lib.vsl_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert 'T=4097 > 4096 clips' in msg, msg


@pytest.mark.gpu
def test_module_trains_one_step_at_1500_clips():
    from vslnet_amd.model.VSLNet import VSLNet
    T = 1500
    cfg = _cfg(T)
    P = O.random_params(cfg, seed=81)
    b = O.synthetic_batch(cfg, 2, T, 9, 6, seed=82, ragged=True)
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
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    before = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    opt.step()
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert any(not torch.equal(before[n], p.detach()) for n, p in m.named_parameters() if p.requires_grad)


# the slab path (VSL_ATTN_DQ_SLABS=1) is read once per process: a child computes its gradients
SLAB_T, SLAB_B = 2048, 2


def _slab_case(num_heads):
    cfg = _cfg(SLAB_T, num_heads, drop_rate=0.2)
    P = O.random_params(cfg, seed=91)
    b = O.synthetic_batch(cfg, SLAB_B, SLAB_T, 9, 6, seed=92, ragged=True)
    eng, flat = _engine(cfg, P)
    return _train_grads(eng, flat, P, _dev(b), 0, SLAB_B, SLAB_B, 1234, float(b['v_mask'].sum())).cpu(), eng


def _slab_child(num_heads, path):
    g, _ = _slab_case(num_heads)
    np.save(path, g.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [8, 16])
def test_slab_switch_gives_the_same_gradients(num_heads, tmp_path):
    out = str(tmp_path / 'slab.npy')
    env = dict(os.environ, VSL_ATTN_DQ_SLABS='1')
    code = 'import sys; sys.path.insert(0, %r); from tests.test_long_video import _slab_child; _slab_child(%d, %r)' % (ROOT, num_heads, out)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    slab = torch.from_numpy(np.load(out))
    g, eng = _slab_case(num_heads)
    for k, t in eng.views(g).items():
        err = float((t - eng.views(slab)[k]).abs().max())
        assert err <= 1e-5 * float(t.abs().max()) + 1e-7, (k, err)
