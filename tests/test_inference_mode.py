"""Inference mode (vsl_io.inference): forward kernels that save nothing + the forward-only workspace plan.

CPU: the ABI (export, version, struct size).  GPU: the mode returns the saved path's bits at every forward dispatch boundary, meets the
reference's goldens on its own, holds four times the batch the training plan holds at T = 4096, needs at most a third (transformer) / half
(rnn) of the training workspace, fails loudly when misused, and is what the module and the evaluation loop take under eval() + no_grad()."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import ROOT, check_routes, extreme_ragged, header_fields, header_sizeof, load_golden
from tests.test_dispatch_boundaries import ROUTE_LABELS, predicted_routes

# the labels of ROUTE_LABELS that are forward launches (forward.hip forward_full / enc_fwd)
FWD_LABELS = tuple(n for n in ROUTE_LABELS if not n.endswith('_bwd'))


# ------------------------------------------------------------------------------------------------ 1. the ABI (CPU)
def _header():
    return open(os.path.join(ROOT, 'include', 'vslnet_hip.h')).read()


def test_library_exports_the_inference_entry_and_abi_9():
    from vslnet_amd import build
    from vslnet_amd.engine import ABI_SYMBOLS, ABI_VERSION
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, 'vsl_inference_workspace_floats')
    assert 'vsl_inference_workspace_floats' in ABI_SYMBOLS
    assert lib.vsl_abi_version() == 9 == ABI_VERSION
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', _header())


def test_ctypes_vsl_io_has_the_size_and_field_order_of_the_header():
    from vslnet_amd import engine
    names = header_fields('vsl_io')                                 # field names, in order, from the header's struct body
    assert names == [f[0] for f in engine.vsl_io._fields_], names
    assert names[-1] == 'inference'
    # the sizes, from the host compiler (every offset of every struct: tests/test_abi_layout.py)
    assert ctypes.sizeof(engine.vsl_io) == header_sizeof('vsl_io')
    assert ctypes.sizeof(engine.vsl_config) == header_sizeof('vsl_config')


# ------------------------------------------------------------------------------------------------ 2. same bits as the saved path
def case(cid, B, T, Lq, heads=8, predictor='transformer', Dv=64, word_dim=300, ragged=False, bf16=False, word_table=False, Lc=6):
    return pytest.param(dict(B=B, T=T, Lq=Lq, heads=heads, predictor=predictor, Dv=Dv, word_dim=word_dim, ragged=ragged, bf16=bf16,
                             word_table=word_table, Lc=Lc), id=cid)


CASES = [
    case('T9-Lq1', 3, 9, 1),
    case('T31-Lq9', 5, 31, 9),
    case('T64-Lq32-last-sample-local-query', 3, 64, 32),
    case('T117-Lq33-row-tile-query-cq-col', 3, 117, 33),
    case('T128-last-attn-block-extreme', 3, 128, 9, ragged=True),
    case('T129-first-split-attention', 3, 129, 9),
    case('T256-Lq40', 2, 256, 40),
    case('T257-key-pairs', 2, 257, 9),
    case('T1024', 2, 1024, 9),
    case('T1025', 2, 1025, 9),
    case('T256-Dv4096-Lq20', 1, 256, 20, Dv=4096, Lc=10),
    case('wd52-fp32-input-linear-Lq40', 3, 56, 40, word_dim=52),
    case('H1-T129-Lq33', 3, 129, 33, heads=1),
    case('H1-T31-Lq1', 3, 31, 1, heads=1),
    case('H2-T64-Lq9-extreme', 3, 64, 9, heads=2, ragged=True),
    case('H2-T257-Lq9', 2, 257, 9, heads=2),
    case('H4-T257-Lq9', 2, 257, 9, heads=4),
    case('H4-T128-Lq32', 3, 128, 32, heads=4),
    case('H16-T128-Lq40', 3, 128, 40, heads=16),
    case('H16-T1025-Lq9', 2, 1025, 9, heads=16),
    case('rnn-B80-one-launch', 80, 16, 6, predictor='rnn'),
    case('rnn-B81-chunked-lstm', 81, 16, 6, predictor='rnn'),
    case('rnn-B81-T128-three-chunks', 81, 128, 9, predictor='rnn'),
    case('rnn-B257-four-sample-groups', 257, 16, 6, predictor='rnn'),
    case('rnn-B3-T129', 3, 129, 9, predictor='rnn'),
    case('rnn-H4-B3-T64-Lq33', 3, 64, 33, predictor='rnn', heads=4),
    case('bf16-features-T128', 3, 128, 9, bf16=True),
    case('bf16-features-T256-Lq33', 2, 256, 33, bf16=True),
    case('word-table-T64', 3, 64, 9, word_table=True),
    case('word-table-T129-Lq33', 3, 129, 33, word_table=True),
]


def _fwd_routes(r):
    want, _ = predicted_routes(r['B'], r['T'], r['Lq'], r['heads'], r['predictor'])
    return tuple(sorted(n for n in want if n in FWD_LABELS))


def test_the_cases_cross_every_forward_boundary_and_route():
    rows = [p.values[0] for p in CASES]
    assert {r['T'] for r in rows} >= {9, 31, 64, 117, 128, 129, 256, 257, 1024, 1025}
    assert {r['Lq'] for r in rows} >= {1, 9, 32, 33, 40}
    assert {r['heads'] for r in rows} == {1, 2, 4, 8, 16}
    assert {r['predictor'] for r in rows} == {'rnn', 'transformer'}
    assert any(r['B'] == 81 and r['predictor'] == 'rnn' for r in rows)
    assert any(r['bf16'] for r in rows) and any(r['word_table'] for r in rows) and any(r['ragged'] for r in rows)
    seen = set()
    for r in rows:
        seen |= set(_fwd_routes(r))
    assert seen == set(FWD_LABELS), sorted(set(FWD_LABELS) - seen)      # a moved threshold cannot empty the table: the GPU test asserts each row's ledger


def _setup(r, param_seed=301, batch_seed=302):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg = O.make_cfg(max_pos_len=max(r['T'], r['Lq']), word_size=102, num_heads=r['heads'], predictor=r['predictor'], video_feature_dim=r['Dv'],
                     word_dim=r['word_dim'], **({'word_table': True} if r['word_table'] else {}))
    P = O.random_params(cfg, seed=param_seed)
    b = O.synthetic_batch(cfg, r['B'], r['T'], r['Lq'], r['Lc'], seed=batch_seed, ragged=True)
    if r['ragged']:
        b = extreme_ragged(b)
    d = {k: v.cuda().contiguous() for k, v in b.items()}
    if r['bf16']:
        d['vfeats'] = d['vfeats'].to(torch.bfloat16)
    eng = Engine(cfg)
    flat = flat_from_state_dict(eng, P)
    pad, glove = P.get('embedding_net.word_emb.pad_vec'), P.get('embedding_net.word_emb.glove_vec')
    args = (flat, None if pad is None else pad.cuda(), None if glove is None else glove.cuda(), d['word_ids'], d['char_ids'], d['vfeats'],
            d['v_mask'], d['q_mask'])
    return cfg, P, b, d, eng, args


def _forward_with_ledger(eng, args, **kw):
    eng.profile_select('*')
    try:
        out = [t.clone() for t in eng.forward(*args, **kw)]
        torch.cuda.synchronize()
        names = [x['name'] for x in eng.profile_launches()]
    finally:
        eng.profile_select(None)
    return out, names


@pytest.mark.gpu
@pytest.mark.parametrize('r', CASES)
def test_inference_forward_has_the_bits_of_the_saved_path(r, request):
    cid = request.node.callspec.id
    cfg, P, b, d, eng, args = _setup(r)
    want = _fwd_routes(r)
    never = tuple(n for n in FWD_LABELS if n not in want)
    saved, names_s = _forward_with_ledger(eng, args, training=False)
    si_s, ei_s = eng.extract_index(saved[1], saved[2])
    infer, names_i = _forward_with_ledger(eng, args, inference=True)
    si_i, ei_i = eng.extract_index(infer[1], infer[2])
    check_routes(names_s, want, never, context=cid + ' (saved path)')
    check_routes(names_i, want, never, context=cid + ' (inference)')
    assert names_i == names_s, (cid, names_s, names_i)              # the same launches under the same labels
    for nm, a, c in zip(('h_score', 'start_logits', 'end_logits'), saved, infer):
        assert torch.equal(a, c), '%s: %s differs, max |diff| %g' % (cid, nm, float((a - c).abs().max()))
    assert torch.equal(si_s, si_i) and torch.equal(ei_s, ei_i), cid
    pad = d['v_mask'] == 0
    assert bool((infer[1][pad] == -1e30).all()) and bool((infer[2][pad] == -1e30).all()) and bool((infer[0][pad] == 0).all()), cid
    # once more, after the saved path has dirtied the whole (larger) workspace: the reused buffers carry nothing over
    again = [t.clone() for t in eng.forward(*args, inference=True)]
    assert all(torch.equal(a, c) for a, c in zip(infer, again)), cid


# ------------------------------------------------------------------------------------------------ 3. against the reference's numbers
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['real_tf', 'long_tf', 'tiny_rnn'])
def test_inference_forward_matches_the_reference_goldens(name):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg, P, b, z = load_golden(name)
    eng = Engine(cfg)
    flat = flat_from_state_dict(eng, P)
    d = {k: v.cuda().contiguous() for k, v in b.items()}
    h, sl, el = eng.forward(flat, P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda(), d['word_ids'],
                            d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], inference=True)
    assert eng._last.inference == 1 and eng.inference_forwards == 1
    h, sl, el = (t.cpu().numpy() for t in (h, sl, el))
    fin = np.abs(z['out.start_logits']) < 1e29
    scale = max(1.0, float(np.abs(z['out.start_logits'][fin]).max()), float(np.abs(z['out.end_logits'][fin]).max()))
    es, ee, eh = (float(np.abs(sl - z['out.start_logits'])[fin].max()), float(np.abs(el - z['out.end_logits'])[fin].max()),
                  float(np.abs(h - z['out.h_score']).max()))
    print('%s: start %.3g end %.3g (gate %.3g), h_score %.3g (gate 2e-5)' % (name, es, ee, 1e-4 * scale, eh))
    assert es < 1e-4 * scale and ee < 1e-4 * scale
    assert eh < 2e-5
    pad = b['v_mask'].numpy() == 0
    assert np.all(sl[pad] == np.float32(-1e30)) and np.all(el[pad] == np.float32(-1e30)) and np.all(h[pad] == 0.0)
    si, ei = eng.extract_index(torch.from_numpy(sl).cuda(), torch.from_numpy(el).cuda())
    assert np.array_equal(si.cpu().numpy(), z['out.start_index']) and np.array_equal(ei.cpu().numpy(), z['out.end_index'])


# ------------------------------------------------------------------------------------------------ 4. capacity
@pytest.mark.gpu
def test_inference_holds_four_times_the_batch_of_the_training_plan_at_4096_clips():
    """The shape of tools/long_rate.py (Dv 64, 8 heads, transformer, T 4096, Lq 20, Lc 10): the training plan stops at the 2^31-float limit,
    the inference plan holds four times the largest power-of-two batch it takes, and that one forward equals the saved-path evaluation
    forwards of its four quarters sample for sample (evaluation is sample-local, the row-tile kernels do not depend on B)."""
    from vslnet_amd.engine import Engine, VslError, flat_from_state_dict
    T, Lq, Lc = 4096, 20, 10
    cfg = O.make_cfg(video_feature_dim=64, num_heads=8, predictor='transformer', max_pos_len=T, word_size=102)
    eng = Engine(cfg)
    refused = 1
    while True:
        try:
            eng.workspace_floats(refused, T, Lq, Lc)
        except VslError as e:
            assert '2^31' in str(e), str(e)
            break
        refused *= 2
        assert refused <= 1024
    hold = refused // 2
    print('training plan: holds B = %d, refuses B = %d' % (hold, refused))
    assert refused <= 32, 'the training plan was expected to stop at B = 32 at the latest (profiles/long_rate.txt: 16 is the largest it holds)'
    Bi = 4 * hold
    n_inf, n_train = eng.inference_workspace_floats(Bi, T, Lq, Lc), eng.workspace_floats(hold, T, Lq, Lc)
    print('inference plan at B = %d: %d floats (%.2f GiB) ; training plan at B = %d: %d floats (%.2f GiB)' % (Bi, n_inf, n_inf * 4 / 2 ** 30, hold, n_train, n_train * 4 / 2 ** 30))
    assert n_inf < 2 ** 31
    P = O.random_params(cfg, seed=401)
    flat = flat_from_state_dict(eng, P)
    pad, glove = P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda()
    b = O.synthetic_batch(cfg, Bi, T, Lq, Lc, seed=402, ragged=True)
    for q in range(4):
        b['lens'][q * hold] = T                      # every quarter keeps the batch's padded T (its own collate would narrow it)
        b['vfeats'][q * hold] = torch.randn(T, 64, generator=torch.Generator().manual_seed(500 + q))
    b['v_mask'] = O.convert_length_to_mask(b['lens'])
    d = {k: b[k].cuda().contiguous() for k in ('word_ids', 'char_ids', 'vfeats', 'v_mask', 'q_mask')}
    full = [t.clone() for t in eng.forward(flat, pad, glove, d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], inference=True)]
    si, ei = (t.clone() for t in eng.extract_index(full[1], full[2]))
    torch.cuda.synchronize()
    for q in range(4):
        s = slice(q * hold, (q + 1) * hold)
        part = eng.forward(flat, pad, glove, d['word_ids'][s].contiguous(), d['char_ids'][s].contiguous(), d['vfeats'][s].contiguous(),
                           d['v_mask'][s].contiguous(), d['q_mask'][s].contiguous(), training=False)
        for nm, a, c in zip(('h_score', 'start_logits', 'end_logits'), full, part):
            assert torch.equal(a[s], c), 'quarter %d: %s differs, max |diff| %g' % (q, nm, float((a[s] - c).abs().max()))
        psi, pei = eng.extract_index(part[1], part[2])
        assert torch.equal(si[s], psi) and torch.equal(ei[s], pei), q


# ------------------------------------------------------------------------------------------------ 5. workspace size
@pytest.mark.gpu
@pytest.mark.parametrize('predictor,den', [('transformer', 3), ('rnn', 2)])
def test_inference_workspace_is_a_fraction_of_the_training_workspace(predictor, den):
    from vslnet_amd.engine import Engine
    eng = Engine(O.make_cfg(predictor=predictor, max_pos_len=4096, word_size=102))
    for B, T, Lq in ((64, 128, 20), (32, 256, 40), (16, 1024, 20), (2, 4096, 9)):
        n_inf, n_train = eng.inference_workspace_floats(B, T, Lq, 10), eng.workspace_floats(B, T, Lq, 10)
        print('%s B %d T %d Lq %d: inference %d / training %d floats = %.3f' % (predictor, B, T, Lq, n_inf, n_train, n_inf / n_train))
        assert n_inf * den <= n_train, (predictor, B, T, Lq, n_inf, n_train)


# ------------------------------------------------------------------------------------------------ 6. misuse fails loudly
@pytest.mark.gpu
def test_misuse_fails_loudly_and_training_after_inference_is_unchanged():
    from vslnet_amd.engine import VslError
    r = dict(B=4, T=96, Lq=9, heads=8, predictor='transformer', Dv=64, word_dim=300, ragged=False, bf16=False, word_table=False, Lc=6)
    cfg, P, b, d, eng, args = _setup(r)
    with pytest.raises(ValueError):
        eng.forward(*args, inference=True, training=True)

    def step():
        eng.forward(*args, training=False)
        losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
        g = eng.backward(d_h, d_sl, d_el, eng.new_flat()).clone()
        return losses.clone(), g
    l0, g0 = step()
    assert eng.ws_view('gated', (r['B'], r['T'], 128)).shape == (r['B'], r['T'], 128)
    h, sl, el = eng.forward(*args, inference=True)
    with pytest.raises(VslError, match='saved nothing'):
        eng.backward(torch.zeros_like(h), torch.zeros_like(sl), torch.zeros_like(el), eng.new_flat())
    with pytest.raises(VslError, match='saves nothing'):
        eng.ws_view('gated', (r['B'], r['T'], 128))
    # the library refuses on its own too (a caller that keeps its own vsl_io): backward in the workspace of an inference forward, tap offsets
    import ctypes as C
    from vslnet_amd.engine import vsl_io
    io = vsl_io()
    C.memmove(C.byref(io), C.byref(eng._last), C.sizeof(vsl_io))
    io.inference = 0
    z = torch.zeros_like(sl)
    g = eng.new_flat()
    io.d_start_logits, io.d_end_logits, io.grads = z.data_ptr(), z.data_ptr(), g.data_ptr()
    assert eng.lib.vsl_backward(eng.h, C.byref(io), None) != 0 and b'saved nothing' in eng.lib.vsl_last_error()
    assert eng.lib.vsl_workspace_offset(eng.h, r['B'], r['T'], r['Lq'], r['Lc'], b'gated') < 0 and b'saved nothing' in eng.lib.vsl_last_error()
    # the eager loss works on an inference forward's outputs
    li = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0, want_grads=False)[0]
    assert torch.allclose(li, l0, rtol=1e-6, atol=0)
    # a lazy loss that is pending when an inference forward arrives is issued first (its scratch lies in the workspace the forward overwrites)
    eng.forward(*args, training=False)
    lz = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0, inv_batch=1.0 / r['B'], mask_sum=float(b['v_mask'].sum()), lazy=True)[0]
    eng.forward(*args, inference=True)
    torch.cuda.synchronize()
    assert abs(float(lz[2]) - float(l0[2])) <= 1e-5 * max(1.0, abs(float(l0[2])))
    # and the next training step is the one it would have been
    l1, g1 = step()
    assert torch.allclose(l0, l1, rtol=1e-6, atol=0) and torch.equal(g0, g1)
    assert eng.ws_view('gated', (r['B'], r['T'], 128)).shape == (r['B'], r['T'], 128)


# ------------------------------------------------------------------------------------------------ 7. the module and the evaluation loop
def _module(cfg, P):
    from model.VSLNet import VSLNet
    m = VSLNet(cfg, np.zeros((cfg.word_size - 2, cfg.word_dim), np.float32))
    m.load_state_dict(P, strict=True)
    return m


@pytest.mark.gpu
def test_module_takes_the_inference_path_under_eval_and_no_grad():
    cfg, P, b, z = load_golden('real_tf')
    m = _module(cfg, P).to('cuda')
    d = {k: v.cuda() for k, v in b.items()}
    inp = (d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'])
    m.eval()
    ref = m(*inp)                                    # eval() with grad enabled: the saved path, a backward may follow
    eng = m._engine
    assert eng.inference_forwards == 0 and eng._last.inference == 0 and all(t.grad_fn is not None for t in ref)
    with torch.no_grad():
        out = m(*inp)
    assert eng.inference_forwards == 1 and eng._last.inference == 1
    assert all(t.grad_fn is None and not t.requires_grad for t in out)
    assert all(torch.equal(a.detach(), c) for a, c in zip(ref, out))
    with pytest.raises(RuntimeError):                # the graph of `ref` points at saves the inference forward has overwritten
        (ref[1].sum() + ref[2].sum() + ref[0].sum()).backward()
    # the saved path again, and its backward runs
    h, sl, el = m(*inp)
    (m.compute_loss(sl, el, d['s_labels'], d['e_labels']) + 5.0 * m.compute_highlight_loss(h, d['h_labels'], d['v_mask'])).backward()
    # train() under no_grad keeps the training path (dropout on)
    cfg2 = O.make_cfg(**{**vars(cfg), 'drop_rate': 0.2})
    m2 = _module(cfg2, P).to('cuda').train()
    with torch.no_grad():
        tr = m2(*inp)
    assert m2._engine.inference_forwards == 0 and m2._engine._last.training == 1
    assert not torch.equal(tr[1], out[1])
    # the switch (an older library behaves like this): off -> the saved path, same bits
    m.eval()
    eng.use_inference = False
    with torch.no_grad():
        off = m(*inp)
    assert eng.inference_forwards == 1 and eng._last.inference == 0
    assert all(torch.equal(a, c) for a, c in zip(off, out))


@pytest.mark.gpu
def test_eval_test_returns_the_same_metrics_with_the_mode_forced_off(monkeypatch):
    from model.VSLNet import VSLNet
    from vslnet_amd import engine as E
    from vslnet_amd.data import get_test_loader, synthetic_dataset
    from vslnet_amd.runner import eval_test
    from vslnet_amd.synthetic import make_configs
    configs = make_configs(video_feature_dim=64, max_pos_len=64, word_size=200, char_size=30, batch_size=8, drop_rate=0.2)
    dataset, feats = synthetic_dataset(configs, n_train=8, n_test=40, seed=3)
    torch.manual_seed(5)
    m = VSLNet(configs, dataset['word_vector']).to('cuda').eval()
    loader = get_test_loader(dataset['test_set'], feats, configs)
    on = eval_test(m, loader, 'cuda', epoch=1, global_step=1)
    n_on = m._engine.inference_forwards
    assert n_on == 5
    monkeypatch.setattr(m._engine, 'use_inference', False)
    off = eval_test(m, loader, 'cuda', epoch=1, global_step=1)
    assert m._engine.inference_forwards == n_on
    assert on[:4] == off[:4], (on, off)
    assert isinstance(m._engine, E.Engine)
