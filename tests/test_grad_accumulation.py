"""Gradient accumulation: one optimizer step over K micro-batches (vsl_backward_accumulate, Engine.backward(accumulate=True),
dp.backward_exchange_step(accumulate=, update=), dp.micro_slices, ResidentSplit.shards(micro_batches=K), main.py --accum_steps K).

A micro-batch is a data-parallel shard run in sequence: global loss normalisers, `sample_offset` = its first row, one seed for the step.  The
accumulating backward forms every sum exactly as the overwriting one and adds the bucket's previous value last, one fp32 add per element.

CPU: the export, dp.micro_slices, the data layer's pieces, main.py's refusals.
GPU: (1) the accumulated bucket is (g0 + g1) + g2 of the pieces' own gradients, bit for bit, pads untouched, twice the same; (2) it is the gradient
of the whole batch at the gates of the shard tests; (3) clip and AdamW act on the accumulated bucket and its norm; (4) misuse fails by name;
(5) main.py --accum_steps, and a global batch whose plan is refused run as micro-batches that fit."""
import ctypes
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import ROOT, hip_relu_masks

CUTS = [0, 2, 3, 6]             # B = 6 as three uneven pieces, one of a single sample
SEED = (5 << 33) + 4711


# ------------------------------------------------------------------------------------------------ CPU
def test_header_declares_and_library_exports_the_entry_point():
    from vslnet_amd import build, engine
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vslnet_hip.h')).read(), flags=re.S)
    assert re.search(r'int\s+vsl_backward_accumulate\s*\(\s*vsl_handle\s+h\s*,\s*const\s+vsl_io\s*\*\s*io\s*,\s*const\s+vsl_shared_io\s*\*\s*sh\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;', hdr)
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', hdr)
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, 'vsl_backward_accumulate')
    assert 'vsl_backward_accumulate' in engine.ABI_SYMBOLS and engine.ABI_VERSION == 9


@pytest.mark.parametrize('n,K', [(6, 3), (16, 4), (7, 3), (64, 16), (1024, 32), (5, 5), (3, 8), (1, 4), (0, 2), (9, 1)])
def test_micro_slices_cover_every_row_once_in_even_contiguous_pieces(n, K):
    from vslnet_amd import dp
    sl = dp.micro_slices(n, K)
    assert len(sl) == K
    rows = [r for s in sl for r in range(n)[s]]
    assert rows == list(range(n))                                   # every row exactly once, in order: the pieces are contiguous
    sizes = [len(range(n)[s]) for s in sl]
    assert max(sizes) - min(sizes) <= 1
    assert sizes == sorted(sizes, reverse=True)                     # the larger pieces first, like shard_slice
    assert sizes.count(0) == max(0, K - n)                          # K > rows: the last pieces are empty
    assert sl == [dp.shard_slice(n, j, K) for j in range(K)]
    with pytest.raises(ValueError):
        dp.micro_slices(n, 0)


def test_resident_shards_cut_every_global_batch_from_one_draw_of_the_order():
    """shards(micro_batches=K) on the CPU: the K pieces of each global batch concatenate to the batch shards() yields for the same generator state
    (ONE shuffle per epoch), keep the global widths and carry row0 / lens_global; a last batch smaller than K yields empty pieces."""
    from vslnet_amd import data, dp
    cfg = SimpleNamespace(video_feature_dim=8, max_pos_len=16, word_dim=300, batch_size=8, seed=3)
    dataset, feats = data.synthetic_dataset(cfg, n_train=19, n_test=4, seed=3)          # 19 = 8 + 8 + 3: the last batch has fewer rows than K = 4
    full = list(data.ResidentSplit(dataset['train_set'], feats, cfg, 'cpu', train=True, generator=torch.Generator().manual_seed(7)).shards())
    K = 4
    micro = list(data.ResidentSplit(dataset['train_set'], feats, cfg, 'cpu', train=True, generator=torch.Generator().manual_seed(7)).shards(micro_batches=K))
    assert len(micro) == K * len(full) == 12
    for i, b in enumerate(full):
        pieces = micro[K * i:K * i + K]
        n = len(b['records'])
        assert [p['row0'] for p in pieces] == [s.start for s in dp.micro_slices(n, K)]
        assert [len(p['records']) for p in pieces] == [len(range(n)[s]) for s in dp.micro_slices(n, K)]
        for key in ('vfeats', 'v_mask', 'word_ids', 'char_ids', 's_labels', 'e_labels', 'h_labels'):
            assert torch.equal(torch.cat([p[key] for p in pieces]), b[key]), key      # (the same widths, or cat / equal would fail)
        assert all(np.array_equal(p['lens_global'], b['lens_global']) for p in pieces)
        assert sum((p['records'] for p in pieces), []) == b['records']
    assert [len(p['records']) for p in micro[-K:]] == [1, 1, 1, 0]
    split = data.ResidentSplit(dataset['train_set'], feats, cfg, 'cpu', train=True, generator=torch.Generator().manual_seed(7))
    with pytest.raises(ValueError, match='micro_batches'):
        next(split.shards(0, 2, micro_batches=2))
    with pytest.raises(ValueError, match='micro_batches'):
        next(split.shards(queries_per_video=2, micro_batches=2))
    # the host-side loader path: the same pieces of every collated batch
    loader = [(b['records'], b['vfeats'], torch.from_numpy(b['lens_global']), b['word_ids'], b['char_ids'], b['s_labels'], b['e_labels'], b['h_labels']) for b in full]
    from_loader = list(data.loader_shards(loader, 'cpu', micro_batches=K))
    assert len(from_loader) == len(micro)
    for p, q in zip(from_loader, micro):
        assert p['row0'] == q['row0'] and p['records'] == q['records'] and np.array_equal(p['lens_global'], q['lens_global'])
        for key in ('vfeats', 'v_mask', 'word_ids', 'char_ids', 's_labels', 'e_labels', 'h_labels'):
            assert torch.equal(p[key], q[key]), key
    with pytest.raises(ValueError, match='micro_batches'):
        next(data.loader_shards(loader, 'cpu', 0, 2, micro_batches=2))


@pytest.mark.parametrize('extra,env,words', [
    (['--optimizer', 'torch'], {}, ('--accum_steps', '--optimizer torch', 'autograd')),
    ([], {'WORLD_SIZE': '2', 'RANK': '0', 'LOCAL_RANK': '0'}, ('--accum_steps', 'single-process', 'world = 2')),
    (['--share_videos'], {}, ('--accum_steps', '--share_videos', 'Engine'))])
def test_main_refuses_what_accumulation_does_not_combine_with(extra, env, words, monkeypatch, tmp_path):
    import main
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = ['--task', 'synthetic', '--predictor', 'transformer', '--mode', 'train', '--epochs', '1', '--batch_size', '16', '--accum_steps', '4',
            '--model_dir', str(tmp_path / 'ckpt')]
    with pytest.raises(ValueError) as e:
        main.run(argv + extra, log=lambda *a: None)
    assert all(w in str(e.value) for w in words), str(e.value)
    assert not (tmp_path / 'ckpt').exists()                         # refused before anything was built or written
    with pytest.raises(ValueError, match='at least 1'):
        main.run(argv[:-4] + ['--accum_steps', '0'], log=lambda *a: None)


# ------------------------------------------------------------------------------------------------ GPU: set-up
CASES = {
    'transformer': dict(T=64, Lq=9),
    'T40-off-tile': dict(T=40, Lq=9),
    'rnn': dict(T=64, Lq=9, predictor='rnn'),
    'word_table': dict(T=64, Lq=9, word_table=True),
    'bf16': dict(T=64, Lq=9, bf16=True),
    'T160-separate-attention': dict(T=160, Lq=9),
}


def _setup(T, Lq, Lc=6, B=6, predictor='transformer', word_table=False, bf16=False, Dv=64):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg = O.make_cfg(video_feature_dim=Dv, max_pos_len=max(T, Lq), word_size=52, drop_rate=0.2, predictor=predictor, word_table=word_table)
    P = O.random_params(cfg, seed=31)
    b = O.synthetic_batch(cfg, B, T, Lq, Lc, seed=32, ragged=True)
    d = {k: v.cuda().contiguous() for k, v in b.items()}
    if bf16:
        d['vfeats'] = d['vfeats'].to(torch.bfloat16)
    eng = Engine(cfg)
    pad, glove = P.get('embedding_net.word_emb.pad_vec'), P.get('embedding_net.word_emb.glove_vec')         # absent: trainable word table
    real = torch.zeros(eng.param_floats, dtype=torch.bool, device='cuda')
    for _, off, numel, _ in eng.layout:
        real[off:off + numel] = True
    return SimpleNamespace(cfg=cfg, P=P, b=b, d=d, eng=eng, flat=flat_from_state_dict(eng, P), pad=None if pad is None else pad.cuda(),
                           glove=None if glove is None else glove.cuda(), B=B, T=T, Lq=Lq, real=real, msum=float(b['v_mask'].sum()), predictor=predictor)


def _nan_bucket(s):
    return torch.full((s.eng.param_floats,), float('nan'), device='cuda')


def _piece(s, lo, hi, grads, flat=None, **kw):
    """forward + production loss (lazy: it rides in the backward) + backward of rows [lo, hi) as a shard of the batch -> (grads, losses)"""
    dd = {k: v[lo:hi].contiguous() for k, v in s.d.items()}
    s.eng.forward(s.flat if flat is None else flat, s.pad, s.glove, dd['word_ids'], dd['char_ids'], dd['vfeats'], dd['v_mask'], dd['q_mask'], training=True,
                  seed=SEED, sample_offset=lo)
    losses, d_h, d_sl, d_el = s.eng.loss(dd['s_labels'], dd['e_labels'], dd['h_labels'], 1.0, 5.0, inv_batch=1.0 / s.B, mask_sum=s.msum, lazy=True)
    return s.eng.backward(d_h, d_sl, d_el, grads, **kw), losses


def _accumulated(s, early_event=False):
    """the three pieces into ONE bucket whose pads hold NaN: the first overwrites, the others add"""
    acc = _nan_bucket(s)
    for i, (lo, hi) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        _piece(s, lo, hi, acc, accumulate=i > 0, early_event=torch.cuda.Event() if early_event else None)
    torch.cuda.synchronize()
    return acc


def _own_buckets(s):
    out = [_piece(s, lo, hi, _nan_bucket(s))[0] for lo, hi in zip(CUTS[:-1], CUTS[1:])]
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ GPU 1: the fp32 sum, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize('case', list(CASES))
def test_accumulated_bucket_is_the_fp32_sum_of_the_pieces_bit_for_bit(case):
    s = _setup(**CASES[case])
    real = s.real
    g = _own_buckets(s)
    acc = _accumulated(s)
    want = (g[0][real] + g[1][real]) + g[2][real]                   # the add order of the header: previous value + this call's sum, one fp32 add each
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert all(float(x[real].abs().max()) > 0 for x in g)           # every piece contributes
    assert torch.equal(acc[real], want), (case, float((acc[real] - want).abs().max()))
    assert bool(torch.isnan(acc[~real]).all()), 'an alignment pad of the bucket was written'
    assert torch.equal(_accumulated(s)[real], acc[real]), 'two runs of the same accumulated step differ'
    if case == 'transformer':                                       # the early block holds its accumulated value when the event fires: the same bits
        with_event = _accumulated(s, early_event=True)
        assert s.eng.early_grad_offset() < s.eng.param_floats
        assert torch.equal(with_event[real], acc[real]) and bool(torch.isnan(with_event[~real]).all())
    if case == 'word_table':        # the batch has table rows only the FIRST piece touches (the later calls must leave them) and rows that pieces share
        rows = [set(s.b['word_ids'][lo:hi].flatten().tolist()) - {0} for lo, hi in zip(CUTS[:-1], CUTS[1:])]
        assert (rows[0] - rows[1] - rows[2]) and (rows[0] & (rows[1] | rows[2])), rows


@pytest.mark.gpu
def test_shared_step_accumulates_through_the_same_entry_point():
    """N = 2 videos, B = 4 queries, T = 64: two different shared steps accumulated into one bucket = the fp32 sum of their own gradients."""
    from tests.test_shared_train import _setup as shared_setup, _step_shared, shared_batch
    a = shared_setup(N=2, idx=[0, 1, 1, 0], T=64, Lq=9)
    eng = a.eng
    sb2 = shared_batch(a.cfg, 2, [1, 1, 0, 1], 64, 9, 6, seed=77)                     # another batch for the same engine and parameters
    steps = [a, SimpleNamespace(**dict(vars(a), sb=sb2, d={k: v.cuda().contiguous() for k, v in sb2.items() if torch.is_tensor(v)}))]
    real = torch.zeros(eng.param_floats, dtype=torch.bool, device='cuda')
    for _, off, numel, _ in eng.layout:
        real[off:off + numel] = True

    def run(accumulate):
        out = [] if not accumulate else torch.full((eng.param_floats,), float('nan'), device='cuda')
        for i, s in enumerate(steps):
            *_, seeds = _step_shared(s, lazy=True)
            if accumulate:
                eng.backward(*seeds, out, accumulate=i > 0)
            else:
                out.append(eng.backward(*seeds, torch.full((eng.param_floats,), float('nan'), device='cuda')))
        torch.cuda.synchronize()
        return out
    g = run(False)
    acc = run(True)
    assert not torch.equal(g[0][real], g[1][real])
    assert torch.equal(acc[real], g[0][real] + g[1][real])
    assert bool(torch.isnan(acc[~real]).all())
    assert torch.equal(run(True)[real], acc[real])


# ------------------------------------------------------------------------------------------------ GPU 2: the full-batch gradient
@pytest.mark.gpu
@pytest.mark.parametrize('case', ['transformer', 'T40-off-tile', 'rnn', 'word_table', 'T160-separate-attention'])
def test_accumulated_bucket_is_the_full_batch_gradient(case):
    """Against ONE backward of the whole batch, at the gates of test_hip_training's shard tests: at most 8 ReLU decisions may move between the
    full-batch run and the pieces; 2e-5 |g|inf + 1e-6 per tensor when none moved (summation order only), 1e-3 |g|inf + 1e-6 otherwise."""
    s = _setup(**CASES[case])
    full, _ = _piece(s, 0, s.B, s.eng.new_flat())
    full = full.double().clone()
    full_masks = hip_relu_masks(s.eng, s.B, s.T, s.Lq, s.predictor)
    acc, moved = s.eng.new_flat(), 0
    for i, (lo, hi) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        _piece(s, lo, hi, acc, accumulate=i > 0)
        moved += sum(int((m != f[lo:hi]).sum()) for m, f in zip(hip_relu_masks(s.eng, hi - lo, s.T, s.Lq, s.predictor), full_masks))
    torch.cuda.synchronize()
    rel = 2e-5 if moved == 0 else 1e-3
    worst, va = 0.0, s.eng.views(acc.double())
    for k, t in s.eng.views(full).items():
        worst = max(worst, float((t - va[k]).abs().max()) / (rel * float(t.abs().max()) + 1e-6))
    print('[accumulate] %s: ReLU decisions moved %d, worst error %.3f of the gate (%g |g|inf + 1e-6)' % (case, moved, worst, rel))
    assert moved <= 8, (case, moved)
    assert worst <= 1.0, (case, worst, moved)


# ------------------------------------------------------------------------------------------------ GPU 3: norm and update act on the sum
@pytest.mark.gpu
@pytest.mark.parametrize('case', ['transformer', 'rnn', 'word_table'])
def test_clip_and_adamw_act_on_the_accumulated_bucket(case):
    """The last piece with fused_step (clip_norm 0.05: the clip is active, so the norm decides the update) against the same accumulation followed by
    adamw_step WITHOUT norm_from_backward (the k_sqsum pass over the bucket), and by adamw_step(norm_from_backward=True).  Gates: identical
    gradients; parameters and moments allclose(rtol 1e-5, atol 1e-9); the norm within 4e-6 relative (test_fused_step_matches_backward_then_adamw).
    A reduction that recorded the squares of the last piece's own sums would report that piece's norm: printed, and asserted to lie far outside
    the gate."""
    from vslnet_amd.dp import FlatAdamW
    s = _setup(**CASES[case])
    eng, real = s.eng, s.real
    pieces = list(zip(CUTS[:-1], CUTS[1:]))
    last_alone = float(torch.linalg.vector_norm(_piece(s, *pieces[-1], eng.new_flat())[0][real].double()))
    runs = {}
    for mode in ('fused', 'sqsum', 'from_backward'):
        flat = s.flat.clone()
        opt = FlatAdamW(flat, eng.layout, lr=1e-3, num_train_steps=10, clip_norm=0.05, engine=eng)
        grads, gn = eng.new_flat(), torch.zeros(1, device='cuda')
        for i, (lo, hi) in enumerate(pieces):
            last = i == len(pieces) - 1
            kw = dict(accumulate=i > 0)
            if last and mode == 'fused':
                kw['fused_step'] = opt.fused_step(grad_norm_out=gn)
            _piece(s, lo, hi, grads, flat=flat, **kw)
        if mode != 'fused':
            lr = opt.lr()
            opt.t += 1
            eng.adamw_step(flat, grads, opt.m, opt.v, lr, opt.t, clip_norm=0.05, grad_norm_out=gn, norm_from_backward=mode == 'from_backward')
        torch.cuda.synchronize()
        runs[mode] = (flat[real].clone(), opt.m[real].clone(), opt.v[real].clone(), float(gn), grads[real].clone(), opt.t)
    want = float(torch.linalg.vector_norm(runs['sqsum'][4].double()))
    print('[accumulate] %s: norm of the accumulated bucket %.8f (fp64 of the bucket) | fused %.8f | k_sqsum %.8f | norm_from_backward %.8f | the last piece alone %.8f'
          % (case, want, runs['fused'][3], runs['sqsum'][3], runs['from_backward'][3], last_alone))
    assert want > 0.05                                              # the clip is active
    assert abs(last_alone - want) > 1e-2 * want                     # ... and the last piece's own norm is nowhere near: summing only its squares fails below
    ref = runs['sqsum']
    assert abs(ref[3] - want) <= 4e-6 * want
    for mode in ('fused', 'from_backward'):
        r = runs[mode]
        assert r[5] == ref[5] == 1
        assert torch.equal(r[4], ref[4]), mode
        assert abs(r[3] - ref[3]) <= 4e-6 * ref[3], (mode, r[3], ref[3])
        for x, y, nm in zip(r[:3], ref[:3], ('params', 'exp_avg', 'exp_avg_sq')):
            assert torch.isfinite(x).all(), (mode, nm)
            assert torch.allclose(x, y, rtol=1e-5, atol=1e-9), (mode, nm, float((x - y).abs().max()))
    assert not torch.equal(ref[0], s.flat[real])                    # the step moved the parameters


@pytest.mark.gpu
def test_step_driver_accumulates_without_advancing_the_optimizer_until_the_last_piece():
    """dp.backward_exchange_step(accumulate=, update=): update=False runs the backward only (opt.t stays), the last piece applies the step to the sum:
    the same bits as driving Engine.backward by hand."""
    from vslnet_amd import dp
    s = _setup(**CASES['transformer'])
    eng = s.eng
    pieces = list(zip(CUTS[:-1], CUTS[1:]))
    out = []
    for driver in (False, True):
        flat = s.flat.clone()
        opt = dp.FlatAdamW(flat, eng.layout, lr=1e-3, num_train_steps=10, clip_norm=0.05, engine=eng)
        grads = eng.new_flat()
        for i, (lo, hi) in enumerate(pieces):
            last = i == len(pieces) - 1
            dd = {k: v[lo:hi].contiguous() for k, v in s.d.items()}
            eng.forward(flat, s.pad, s.glove, dd['word_ids'], dd['char_ids'], dd['vfeats'], dd['v_mask'], dd['q_mask'], training=True, seed=SEED, sample_offset=lo)
            _, *seeds = eng.loss(dd['s_labels'], dd['e_labels'], dd['h_labels'], 1.0, 5.0, inv_batch=1.0 / s.B, mask_sum=s.msum, lazy=True)
            if driver:
                dp.backward_exchange_step(eng, None, grads, seeds, opt, accumulate=i > 0, update=last)
                assert opt.t == int(last)
            else:
                eng.backward(*seeds, grads, accumulate=i > 0, fused_step=opt.fused_step() if last else None)
        torch.cuda.synchronize()
        out.append((flat.clone(), grads.clone(), opt.m.clone(), opt.v.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match='skipped by the caller'):
        dp.backward_exchange_step(eng, None, eng.new_flat(), None, opt, accumulate=True, update=False)


# ------------------------------------------------------------------------------------------------ GPU 4: misuse
@pytest.mark.gpu
def test_misuse_fails_by_name_and_leaves_the_engine_usable():
    import ctypes as C
    from vslnet_amd.engine import VslError, vsl_shared_io, _ptr
    from tests.test_shared_train import _setup as shared_setup, _step_shared
    s = _setup(**CASES['transformer'])
    eng = s.eng
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def err(rc):
        assert rc != 0
        return eng.lib.vsl_last_error().decode()
    g_ref = _piece(s, 0, s.B, eng.new_flat())[0].clone()
    # NULL grads
    dd = s.d
    eng.forward(s.flat, s.pad, s.glove, dd['word_ids'], dd['char_ids'], dd['vfeats'], dd['v_mask'], dd['q_mask'], training=True, seed=SEED)
    _, d_h, d_sl, d_el = eng.loss(dd['s_labels'], dd['e_labels'], dd['h_labels'], 1.0, 5.0, inv_batch=1.0 / s.B, mask_sum=s.msum)
    io = eng._last
    io.d_h_score, io.d_start_logits, io.d_end_logits, io.grads = _ptr(d_h), _ptr(d_sl), _ptr(d_el), None
    msg = err(eng.lib.vsl_backward_accumulate(eng.h, C.byref(io), None, stream))
    assert 'vsl_backward_accumulate' in msg and 'grads' in msg, msg
    # a vsl_shared_io behind an ordinary forward
    bucket = eng.new_flat()
    io.grads = _ptr(bucket)
    sh = vsl_shared_io()
    vidx, vmask = torch.zeros(s.B, dtype=torch.int32, device='cuda'), dd['v_mask'][:1].contiguous()
    sh.N, sh.video_index, sh.video_v_mask = 1, _ptr(vidx), _ptr(vmask)
    msg = err(eng.lib.vsl_backward_accumulate(eng.h, C.byref(io), C.byref(sh), stream))
    assert 'vsl_backward_accumulate' in msg and 'not vsl_forward_shared' in msg, msg
    # after an inference forward: nothing was saved (the binding refuses first; the library by itself too)
    eng.forward(s.flat, s.pad, s.glove, dd['word_ids'], dd['char_ids'], dd['vfeats'], dd['v_mask'], dd['q_mask'], inference=True)
    with pytest.raises(VslError, match='inference forward'):
        eng.backward(d_h, d_sl, d_el, bucket, accumulate=True)
    io2 = eng._last
    io2.d_h_score, io2.d_start_logits, io2.d_end_logits, io2.grads = _ptr(d_h), _ptr(d_sl), _ptr(d_el), _ptr(bucket)
    msg = err(eng.lib.vsl_backward_accumulate(eng.h, C.byref(io2), None, stream))
    assert 'vsl_backward_accumulate' in msg and 'the last forward saved nothing' in msg, msg
    # a library without the symbol
    eng.forward(s.flat, s.pad, s.glove, dd['word_ids'], dd['char_ids'], dd['vfeats'], dd['v_mask'], dd['q_mask'], training=True, seed=SEED)
    eng.has_grad_accumulation = False
    with pytest.raises(VslError, match='vsl_backward_accumulate is missing'):
        eng.backward(d_h, d_sl, d_el, bucket, accumulate=True)
    eng.has_grad_accumulation = True
    torch.cuda.synchronize()
    assert float(bucket.abs().max()) == 0.0                         # no refused call wrote the bucket
    # ... and a plain step afterwards is the one from before the refusals, bit for bit
    g_after = _piece(s, 0, s.B, eng.new_flat())[0]
    torch.cuda.synchronize()
    assert torch.equal(g_after, g_ref)
    # NULL sh behind a shared forward
    a = shared_setup(N=2, idx=[0, 1, 1, 0], T=64, Lq=9)
    *_, seeds = _step_shared(a)
    io3 = a.eng._last
    g3 = a.eng.new_flat()
    io3.d_h_score, io3.d_start_logits, io3.d_end_logits, io3.grads = _ptr(seeds[0]), _ptr(seeds[1]), _ptr(seeds[2]), _ptr(g3)
    rc = a.eng.lib.vsl_backward_accumulate(a.eng.h, C.byref(io3), None, stream)
    msg = a.eng.lib.vsl_last_error().decode()
    assert rc != 0 and 'vsl_backward_accumulate' in msg and 'vsl_forward_shared' in msg, msg
    plain = a.eng.backward(*seeds, a.eng.new_flat()).clone()
    *_, seeds = _step_shared(a)
    again = a.eng.backward(*seeds, a.eng.new_flat())
    torch.cuda.synchronize()
    assert torch.equal(plain, again)


# ------------------------------------------------------------------------------------------------ GPU 5: the command line, and a batch that does not fit
@pytest.mark.gpu
def test_main_accum_steps_takes_the_same_steps_and_starts_from_the_same_loss(tmp_path):
    """--accum_steps 4 against 1 at the same seed: the same number of optimizer steps and num_train_steps; the step-1 loss -- taken before any update,
    the sum of the four pieces' partial sums of the global loss -- within 2e-5 (summation order only); a finite last loss and a checkpoint."""
    import main
    base = ['--task', 'synthetic', '--predictor', 'transformer', '--batch_size', '16', '--epochs', '1', '--mode', 'train', '--max_pos_len', '32',
            '--video_feature_dim', '64', '--synthetic_train', '64', '--synthetic_test', '16', '--period', '1']
    outs = {}
    for K in (1, 4):
        out = main.run(base + ['--accum_steps', str(K), '--model_dir', str(tmp_path / ('ckpt%d' % K))], log=lambda *a: None)
        with open(os.path.join(out['model_dir'], 'configs.json')) as f:
            out['configs'] = json.load(f)
        out['losses'] = [v for _, v in out['history'] if isinstance(v, float)]
        outs[K] = out
    a, b = outs[1], outs[4]
    assert a['steps'] == b['steps'] == 4 and a['configs']['num_train_steps'] == b['configs']['num_train_steps'] == 4
    assert b['configs']['accum_steps'] == 4 and a['configs']['accum_steps'] == 1
    assert len(a['losses']) == len(b['losses']) == 4
    print('[accumulate] main.py step-1 loss: --accum_steps 1 %.7f, --accum_steps 4 %.7f (difference %.2e); last %.5f / %.5f'
          % (a['losses'][0], b['losses'][0], abs(a['losses'][0] - b['losses'][0]), a['losses'][-1], b['losses'][-1]))
    assert abs(a['losses'][0] - b['losses'][0]) <= 2e-5, (a['losses'][0], b['losses'][0])
    assert all(np.isfinite(b['losses']))
    assert any(f.endswith('.t7') for f in os.listdir(b['model_dir']))


@pytest.mark.gpu
def test_a_global_batch_whose_plan_is_refused_runs_as_micro_batches_that_fit():
    """The 2^31-float limit applies to the micro-batch's shape.  The smallest global batch vsl_workspace_floats refuses at T = 64 (found by bisection)
    is cut into micro-batches of 4 or 5 rows; the first TWO of them run as pieces of that batch (its 1 / B, a mask sum of its size, their own
    sample_offset) and accumulate to the fp32 sum of their own gradients."""
    from vslnet_amd import dp
    from vslnet_amd.engine import VslError
    T, Lq, Lc = 64, 5, 4
    s = _setup(T=T, Lq=Lq, Lc=Lc, B=10, Dv=16)                        # (the rows of the two pieces that run; the rest of the batch is never built)
    eng = s.eng

    def fits(B):
        try:
            eng.workspace_floats(B, T, Lq, Lc)
            return True
        except VslError as e:
            assert '2^31' in str(e) or '2 GiB' in str(e), str(e)
            return False
    lo, hi = 8, 1 << 16
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    Bg = hi                                                         # the smallest refused batch; Bg - 1 fits
    rows = [(c.start, c.stop) for c in dp.micro_slices(Bg, Bg // 4)[:2]]
    assert rows[0][0] == 0 and rows[1][1] <= 10 and all(b - a in (4, 5) for a, b in rows), rows
    for a, b in rows:
        eng.workspace_floats(b - a, T, Lq, Lc)                      # the micro shape fits
    print('[accumulate] T=%d: the training plan is refused from B=%d on; running rows %s of it' % (T, Bg, rows))
    s.B, s.msum = Bg, 0.75 * Bg * T                                 # the global normalisers of a batch of Bg samples
    own = [_piece(s, a, b, _nan_bucket(s))[0] for a, b in rows]
    acc = _nan_bucket(s)
    for i, (a, b) in enumerate(rows):
        _piece(s, a, b, acc, accumulate=i > 0)
    torch.cuda.synchronize()
    want = own[0][s.real] + own[1][s.real]
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(acc[s.real], want)
    assert bool(torch.isnan(acc[~s.real]).all())
