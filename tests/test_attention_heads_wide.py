"""num_heads 1 and 2 (head sizes 128 and 64): the attention core of kernels_attn_wide.hip (shared parts: attn.hpp; dispatch: kernels_attn.hip), through every layer above it.

CPU-only tests: vsl_create's head-count validation (it runs before the device query) and the oracle against fixtures the reference
itself produced with 1 and 2 heads (tools/make_golden_heads.py; each fixture is split into files under 1 MiB).
GPU tests: eval-mode parity with those fixtures and with the oracle at every length boundary of the new kernels (16-row tiles, the 256-key
dQ slabs, element hashes -> key pairs at 256/257, slab dQ -> one query-major dQ at 1024/1025), training mode on the same dropout masks,
long videos up to 4096 clips, finite differences, determinism, the data-parallel shard sum, the slab switch, the autograd module, the CLI
and the launch routes.  Gates are those of test_attention_heads.py and test_long_video.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import ROOT, check_training_against_oracle, extreme_ragged, grad_tol
from tests.test_attention_heads import _create, _dev, _engine, _err, _fwd, _grads_vs_oracle, _close, load_heads_golden
from tests.test_long_video import _cfg, _train_grads

WIDE_CASES = {'heads1_tf': 1, 'heads2_tf': 2}
ROUTE_WANT = ('attn_fwd', 'attn_out_fwd', 'attn_bwd')
ROUTE_NEVER = ('attn_block_fwd',)


# ------------------------------------------------------------------------------------------------ vsl_create (no GPU)
@pytest.mark.parametrize('num_heads', [1, 2])
def test_create_accepts_1_and_2_heads(num_heads):
    rc, msg = _create(num_heads)
    if torch.cuda.is_available():
        assert rc == 0, msg
    else:
        assert rc != 0 and 'no HIP device' in msg, msg          # the only refusal left on a machine without a GPU


def test_create_names_every_supported_head_count():
    rc, msg = _create(32)
    assert rc != 0 and 'num_heads=32' in msg and '1, 2, 4, 8 and 16' in msg and '128, 64, 32, 16 and 8' in msg, msg
    for h in (64, 128):
        rc, msg = _create(h)
        assert rc != 0 and 'num_heads=%d' % h in msg, msg
    rc, msg = _create(3)
    assert rc != 0 and 'not a multiple of attention heads' in msg, msg


# ------------------------------------------------------------------------------------------------ oracle vs reference (no GPU)
@pytest.mark.parametrize('name', list(WIDE_CASES))
def test_oracle_reproduces_the_reference_at_1_and_2_heads(name):
    cfg, P, b, z = load_heads_golden(name)
    assert cfg.num_heads == WIDE_CASES[name]
    with torch.no_grad():
        h, sl, el = O.forward(P, cfg, b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'], training=False)
    _close(h, z['out.h_score'], atol=5e-6, what='h_score')
    _close(sl, z['out.start_logits'], what='start_logits')
    _close(el, z['out.end_logits'], what='end_logits')
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
@pytest.mark.gpu
@pytest.mark.parametrize('name', list(WIDE_CASES))
def test_eval_logits_and_gradients_match_the_reference(name):
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
    for what, got, key, atol in [('h_score', h, 'out.h_score', 2e-5), ('start_logits', sl, 'out.start_logits', 1e-4),
                                 ('end_logits', el, 'out.end_logits', 1e-4)]:
        err, tol = _err(got, z[key], atol)
        if not err <= tol:
            bad.append((what, err, tol))
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


# every boundary of the new kernels: below one 16-row tile, 64/65, 128/129, 256/257 (element hashes -> key pairs, one -> two dQ slabs),
# 1024/1025 (four dQ slabs -> one query-major dQ)
EVAL_SHAPES = [(3, 9, 7, 'transformer'), (3, 64, 7, 'transformer'), (3, 65, 40, 'rnn'), (2, 128, 20, 'transformer'), (2, 129, 9, 'transformer'),
               (2, 256, 7, 'rnn'), (2, 257, 9, 'transformer'), (1, 1024, 7, 'transformer'), (2, 1025, 9, 'transformer')]


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [1, 2])
@pytest.mark.parametrize('B,T,Lq,predictor', EVAL_SHAPES)
def test_eval_mode_matches_oracle(num_heads, B, T, Lq, predictor):
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=max(T, Lq), word_size=52, predictor=predictor, num_heads=num_heads)
    P = O.random_params(cfg, seed=31)
    b = O.synthetic_batch(cfg, B, T, Lq, 6, seed=32, ragged=True)
    eng, flat = _engine(cfg, P)
    bad = _grads_vs_oracle(eng, flat, P, cfg, b, _dev(b))
    assert not bad, bad[:6]


TRAIN_SHAPES = [(3, 11, 7, 'transformer'), (3, 64, 9, 'rnn'), (2, 65, 7, 'transformer'), (2, 128, 20, 'transformer'), (2, 129, 7, 'rnn'),
                (2, 256, 9, 'transformer'), (2, 257, 7, 'transformer'), (1, 1024, 7, 'transformer'), (2, 1025, 7, 'transformer')]


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [1, 2])
@pytest.mark.parametrize('B,T,Lq,predictor', TRAIN_SHAPES)
def test_training_mode_matches_oracle_on_the_same_dropout_masks(num_heads, B, T, Lq, predictor):
    check_training_against_oracle(B, T, Lq, 6, cfg=dict(video_feature_dim=64, predictor=predictor, num_heads=num_heads), param_seed=21,
                                  batch_seed=22, step_seed=(7 << 33) + 12345, want=ROUTE_WANT, never=ROUTE_NEVER,
                                  context='num_heads=%d T=%d' % (num_heads, T))


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [1, 2])
@pytest.mark.parametrize('T', [100, 300])
def test_training_mode_on_an_extreme_ragged_batch(num_heads, T):
    check_training_against_oracle(3, T, 9, 6, cfg=dict(video_feature_dim=64, num_heads=num_heads), param_seed=23, batch_seed=24,
                                  step_seed=(3 << 33) + 777, transform=extreme_ragged, want=ROUTE_WANT, never=ROUTE_NEVER,
                                  context='extreme ragged num_heads=%d T=%d' % (num_heads, T))


# ------------------------------------------------------------------------------------------------ long videos (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [1, 2])
@pytest.mark.parametrize('T,B', [(1500, 2), (2048, 1), (4096, 1)])
def test_eval_mode_matches_oracle_on_long_videos(num_heads, T, B):
    cfg = _cfg(T, num_heads)
    P = O.random_params(cfg, seed=41)
    b = O.synthetic_batch(cfg, B, T, 9, 6, seed=42, ragged=True)
    eng, flat = _engine(cfg, P)
    bad = _grads_vs_oracle(eng, flat, P, cfg, b, _dev(b))
    assert not bad, bad[:6]


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [1, 2])
@pytest.mark.parametrize('T,B', [(1500, 2), (2048, 1)])
def test_training_mode_on_long_videos(num_heads, T, B):
    check_training_against_oracle(B, T, 7, 6, cfg=dict(video_feature_dim=64, num_heads=num_heads), param_seed=51, batch_seed=52,
                                  step_seed=(5 << 33) + 4321)


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [1, 2])
@pytest.mark.parametrize('T', [160, 1100])
def test_dropout_forward_backward_consistency_by_finite_differences(num_heads, T):
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
    # the attention's query projection reaches the loss only through dQ: its own direction checks the dQ kernel
    only_q = torch.zeros_like(gd)
    for n, o, k, _ in eng.layout:
        if n.endswith('attention_block.query.conv1d.weight'):
            only_q[o:o + k] = gd[o:o + k]
    assert float(only_q.norm()) > 0
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


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads,T,B', [(1, 300, 2), (2, 1500, 2), (1, 4096, 1)])
def test_backward_is_bit_identical_across_runs(num_heads, T, B):
    cfg = _cfg(T, num_heads, drop_rate=0.2)
    P = O.random_params(cfg, seed=71)
    b = O.synthetic_batch(cfg, B, T, 9, 6, seed=72, ragged=True)
    d = _dev(b)
    eng, flat = _engine(cfg, P)
    msum = float(b['v_mask'].sum())
    g1 = _train_grads(eng, flat, P, d, 0, B, B, 99, msum)
    g2 = _train_grads(eng, flat, P, d, 0, B, B, 99, msum)
    assert torch.equal(g1, g2)


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [1, 2])
def test_data_parallel_shards_add_up(num_heads):
    """training mode, global normalisers and sample_offset: three uneven shards reproduce the full batch's gradient"""
    from tests.helpers import hip_relu_masks
    B, T, Lq, Lc = 16, 128, 20, 10
    cfg = O.make_cfg(video_feature_dim=256, max_pos_len=T, word_size=1002, drop_rate=0.2, num_heads=num_heads)
    P = O.random_params(cfg, seed=12345)
    b = O.synthetic_batch(cfg, B, T, Lq, Lc, seed=0, ragged=True)
    d = _dev(b)
    eng, flat = _engine(cfg, P)
    seed, msum = 20260928, float(b['v_mask'].sum())
    full = _train_grads(eng, flat, P, d, 0, B, B, seed, msum)
    fm = hip_relu_masks(eng, B, T, Lq)
    parts = torch.zeros_like(full)
    moved = 0
    for lo, hi in [(0, 6), (6, 10), (10, B)]:
        parts += _train_grads(eng, flat, P, d, lo, hi, B, seed, msum)
        moved += sum(int((a != f[lo:hi]).sum()) for a, f in zip(hip_relu_masks(eng, hi - lo, T, Lq), fm))
    assert moved == 0, moved
    for k, t in eng.views(full).items():
        err = float((t - eng.views(parts)[k]).abs().max())
        assert err <= 2e-5 * float(t.abs().max()) + 1e-6, (k, err)


@pytest.mark.gpu
@pytest.mark.parametrize('num_heads', [1, 2])
def test_slab_switch_gives_the_same_gradients(num_heads, tmp_path):
    """VSL_ATTN_DQ_SLABS=1 (read once per process, so in a child): the dQ kernel writes 256-key partial slabs at T = 2048 too"""
    from tests.test_long_video import _slab_case
    out = str(tmp_path / 'slab.npy')
    env = dict(os.environ, VSL_ATTN_DQ_SLABS='1')
    code = 'import sys; sys.path.insert(0, %r); from tests.test_long_video import _slab_child; _slab_child(%d, %r)' % (ROOT, num_heads, out)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    slab = torch.from_numpy(np.load(out))
    g, eng = _slab_case(num_heads)
    # the floor is the parity gate's 1e-6: the key projection's bias gradient is zero in exact arithmetic (softmax is shift-invariant per
    # query), so what it holds is rounding noise (~1e-7 at one head) that the changed dQ summation order redraws
    for k, t in eng.views(g).items():
        err = float((t - eng.views(slab)[k]).abs().max())
        assert err <= 1e-5 * float(t.abs().max()) + 1e-6, (k, err)


# ------------------------------------------------------------------------------------------------ module and CLI (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize('name', list(WIDE_CASES))
def test_module_matches_the_engine(name):
    from vslnet_amd.model.VSLNet import VSLNet
    cfg, P, b, z = load_heads_golden(name)
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


@pytest.mark.gpu
def test_cli_trains_one_epoch_with_1_head(tmp_path):
    argv = [sys.executable, os.path.join(ROOT, 'main.py'), '--task', 'synthetic', '--num_heads', '1', '--epochs', '1', '--max_pos_len', '32',
            '--video_feature_dim', '64', '--batch_size', '16', '--synthetic_train', '64', '--synthetic_test', '32', '--period', '1',
            '--model_dir', str(tmp_path)]
    r = subprocess.run(argv, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(line.rsplit('loss', 1)[1]) for line in r.stdout.splitlines() if '| loss' in line]
    assert len(losses) >= 4 and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
