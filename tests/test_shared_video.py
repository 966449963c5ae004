"""One encoding per video, many queries against it: vsl_encode_video + vsl_localize, Engine / VSLNet.encode_video + localize,
ResidentSplit.encode, runner.eval_test_shared.

CPU: the ABI (the four exports, version 9, struct sizes and field orders) and the oracle restatement "encode once, index_select, the rest"
that the GPU numbers are gated against.  GPU: localize on a resident encoding returns the BITS of the inference forward on the replicated batch
at every forward dispatch boundary of the CQ stage and its neighbours; the launch ledger of both calls; the reference's goldens; the workspace
bounds; loud failures on misuse; the evaluation loop.

Finding of the bit-equality run (MI355X).  Every case at a whole-tile T (128, 160, 256, 1024) or T <= 32 is bit-equal.  At a T off the 32-row tile
(117, 300) the outputs are bit-equal only when every video sits at the batch position it was encoded at (idx = arange(N)); otherwise h_score
differs from the inference forward on the replicated batch by 6.6e-7 .. 1.3e-6.  That is a property of an EXISTING kernel, not of the indexed CQ
kernels (measured with saved-path forwards alone, tap by tap): k_convblock_fwd<3, .>, the conv block of launch_cbf<3>, in the DEPTHWISE CONVOLUTION
of conv layer 0 -- x0 is still bit-equal, y0 is the first tap that differs, in at most 32 rows per sample by 2.4e-7.  A workgroup whose 56-row
window crosses a sample boundary takes the per-tap-tested loop (`u += test ? w * x : 0`), every other one the plain loop (`u += w * x`), and the two
do not round alike; which tiles cross a boundary depends on b * T mod 32, i.e. on the sample's position in the batch.  Those cases are gated at
the golden tolerances below (OFF_TILE_MOVED), as DESIGN section 7 records; the encoding itself always equals the saved `venc` of the same N videos."""
import ctypes
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.helpers import ROOT, check_routes, check_training_against_oracle, extreme_ragged, header_fields, header_sizeof, load_golden
from tests.test_dispatch_boundaries import ROUTE_LABELS, predicted_routes

FWD_LABELS = tuple(n for n in ROUTE_LABELS if not n.endswith('_bwd'))
NEW_SYMBOLS = ('vsl_encode_workspace_floats', 'vsl_encode_video', 'vsl_localize_workspace_floats', 'vsl_localize')
PARENT_SIZEOF_VSL_IO = 208      # sizeof(vsl_io) of the commit this feature was added to (ABI 9, `inference` last): the struct must not move


# ------------------------------------------------------------------------------------------------ 1. the ABI (CPU)
def _header():
    return open(os.path.join(ROOT, 'include', 'vslnet_hip.h')).read()


def test_library_exports_the_shared_video_entry_points_and_keeps_abi_9():
    from vslnet_amd import build, engine
    lib = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in engine.ABI_SYMBOLS, s
    assert lib.vsl_abi_version() == 9 == engine.ABI_VERSION
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', _header())
    # (the mirrors of vsl_encode_io and vsl_localize_io against the header and the host compiler: tests/test_abi_layout.py, as for every struct)
    assert ctypes.sizeof(engine.vsl_io) == header_sizeof('vsl_io') == PARENT_SIZEOF_VSL_IO and header_fields('vsl_io')[-1] == 'inference'


# ------------------------------------------------------------------------------------------------ 2. the oracle, restated (CPU)
def oracle_localize(P, cfg, vfeats, v_mask, idx, word_ids, char_ids, q_mask):
    """O.forward with the video half hoisted: the N videos go through VisualProjection and the feature encoder ONCE, the encoding (and the mask)
    are index_select-ed per query, everything else is O.forward's own sequence.  The oracle itself is not edited."""
    p, H = float(cfg.drop_rate), int(cfg.num_heads)
    vf = O.visual_projection(P, vfeats, p, False)
    enc = O.feature_encoder(P, 'feature_encoder.', vf, v_mask, H, p, False, None)
    idx = torch.as_tensor(idx, dtype=torch.int64)
    ve, vm = torch.index_select(enc, 0, idx), torch.index_select(v_mask, 0, idx)
    qf = O.embedding(P, word_ids, char_ids, p, False)
    qe = O.feature_encoder(P, 'feature_encoder.', qf, q_mask, H, p, False, None)
    f1 = O.cq_attention(P, ve, qe, vm, q_mask, p, False, None)
    f2 = O.cq_concat(P, f1, qe, q_mask)
    h = O.highlight(P, f2, vm)
    sl, el = O.conditioned_predictor(P, f2 * h[:, :, None], vm, cfg.predictor, H, p, False, None)
    return h, sl, el, enc


def _videos_and_queries(cfg, N, B, T, Lq, Lc, seed, ragged=True, extreme=False):
    """N videos (features, lengths, mask; video 0 fills T) and B queries, drawn independently.  extreme: the last video shrinks to ONE clip and the
    first query to ONE word (helpers.extreme_ragged on each side)."""
    vb = O.synthetic_batch(cfg, N, T, Lq, Lc, seed=seed, ragged=ragged)
    qb = O.synthetic_batch(cfg, B, T, Lq, Lc, seed=seed + 1, ragged=ragged)
    if extreme:
        vb, qb = extreme_ragged(vb), extreme_ragged(qb)
    assert vb['v_mask'].shape == (N, T) and int(vb['lens'][0]) == T
    return vb, qb


def test_oracle_restatement_equals_the_forward_on_the_replicated_batch():
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=64, word_size=102)
    P = O.random_params(cfg, seed=11)
    idx = [0, 0, 2, 1, 0, 2, 2]
    vb, qb = _videos_and_queries(cfg, 3, len(idx), 64, 9, 6, seed=12)
    with torch.no_grad():
        h, sl, el, _ = oracle_localize(P, cfg, vb['vfeats'], vb['v_mask'], idx, qb['word_ids'], qb['char_ids'], qb['q_mask'])
        rh, rsl, rel = O.forward(P, cfg, qb['word_ids'], qb['char_ids'], vb['vfeats'][idx], vb['v_mask'][idx], qb['q_mask'])
    for nm, a, c in (('h_score', h, rh), ('start_logits', sl, rsl), ('end_logits', el, rel)):
        assert torch.equal(a, c), '%s: max |diff| %g' % (nm, float((a - c).abs().max()))


# ------------------------------------------------------------------------------------------------ 3. the bits of the inference forward (GPU)
def case(cid, N, B, idx, T, Lq, heads=8, predictor='transformer', Dv=64, ragged=True, extreme=False, bf16=False, word_table=False, Lc=6):
    idx = list(idx)
    assert len(idx) == B and min(idx) >= 0 and max(idx) < N
    return pytest.param(dict(N=N, B=B, idx=idx, T=T, Lq=Lq, heads=heads, predictor=predictor, Dv=Dv, ragged=ragged, extreme=extreme, bf16=bf16,
                             word_table=word_table, Lc=Lc), id=cid)


def _cycle(N, B, skip=()):
    """B indices over N videos: every video outside `skip` used, in a scrambled order, with repeats when B > N."""
    use = [v for v in range(N) if v not in skip]
    return [use[(5 * i + i // len(use)) % len(use)] for i in range(B)]


CASES = [
    # N != B, repeated and unused videos (video 0 fills T; with `extreme` the last video has one clip and query 0 one word)
    case('T24-Lq9-under-a-row-tile', 5, 7, [0, 0, 2, 4, 0, 2, 2], 24, 9),                        # fold, sample-local query, score<8>
    case('T117-Lq33-off-tile-cq-col', 4, 6, [0, 3, 3, 1, 0, 3], 117, 33),                        # launch_cbf<3>, cq_col, row-tile query
    case('T117-Lq9-off-tile-fold-extreme', 4, 6, [3, 0, 3, 1, 0, 3], 117, 9, extreme=True),
    case('T128-Lq32-last-fold-extreme', 3, 5, [2, 0, 2, 2, 0], 128, 32, extreme=True),           # cq_col_folds' last shape, heads hosted
    case('T128-Lq33-first-cq-col', 3, 5, [0, 2, 2, 0, 0], 128, 33),
    case('T160-Lq9-split-attention', 3, 4, [0, 2, 0, 2], 160, 9),
    case('T256-Lq70-score12', 2, 3, [1, 0, 1], 256, 70),                                         # k_cq_score<12>, big-Lq k_cq_out
    case('T256-Lq32-extreme', 3, 4, [2, 0, 2, 1], 256, 32, extreme=True),
    case('T300-Lq9-off-tile', 3, 4, [0, 2, 2, 0], 300, 9),
    case('T300-Lq70-off-tile-extreme', 3, 4, [2, 2, 0, 1], 300, 70, extreme=True),
    case('T1024-Lq9', 2, 3, [1, 0, 1], 1024, 9),
    case('T1024-Lq33', 2, 2, [0, 0], 1024, 33),
    # one video for a whole batch of queries, one query against a corpus
    case('N1-B64-T128-Lq9', 1, 64, [0] * 64, 128, 9),
    case('N1-B64-T117-Lq33', 1, 64, [0] * 64, 117, 33),
    case('N64-B1-T128-Lq33', 64, 1, [37], 128, 33),
    case('N64-B1-T24-Lq9', 64, 1, [63], 24, 9),
    # head counts
    case('H4-T128-Lq32', 3, 5, [0, 2, 2, 0, 1], 128, 32, heads=4),
    case('H4-T300-Lq33', 3, 4, [2, 0, 2, 0], 300, 33, heads=4),
    case('H1-T117-Lq70', 3, 4, [0, 2, 2, 1], 117, 70, heads=1),
    case('H1-T24-Lq9-extreme', 3, 4, [2, 0, 2, 1], 24, 9, heads=1, extreme=True),
    # the rnn predictor: one launch (B <= 80) and the chunked LSTMs (B = 96)
    case('rnn-B7-T24-Lq9', 5, 7, [0, 0, 2, 4, 0, 2, 2], 24, 9, predictor='rnn'),
    case('rnn-B80-T117-Lq33', 6, 80, _cycle(6, 80, skip=(4,)), 117, 33, predictor='rnn'),
    case('rnn-B96-T128-Lq9-extreme', 7, 96, _cycle(7, 96, skip=(3,)), 128, 9, predictor='rnn', extreme=True),
    case('rnn-B96-T160-Lq70', 5, 96, _cycle(5, 96, skip=(1,)), 160, 70, predictor='rnn'),
    # off the row tile with every video at the position it was encoded at: bit-equal there too (see the module docstring)
    case('T117-Lq33-same-positions', 4, 4, [0, 1, 2, 3], 117, 33),
    case('T300-Lq9-same-positions-extreme', 3, 3, [0, 1, 2], 300, 9, extreme=True),
    # bf16 features, the trainable word table
    case('bf16-T128-Lq9', 3, 5, [0, 2, 2, 0, 1], 128, 9, bf16=True),
    case('bf16-T256-Lq33-extreme', 3, 4, [2, 0, 2, 1], 256, 33, bf16=True, extreme=True),
    case('word-table-T117-Lq9', 4, 6, [0, 3, 3, 1, 0, 3], 117, 9, word_table=True),
    case('word-table-T160-Lq33', 3, 4, [0, 2, 0, 2], 160, 33, word_table=True),
]


def off_tile_moved(r):
    """The one exception to bit equality (module docstring): T off the 32-row tile AND a video at another batch position than in the encode call --
    k_convblock_fwd<3>'s depthwise conv rounds the rows of a tile that crosses a sample boundary differently.  Gated at the golden tolerances."""
    return r['T'] > 32 and r['T'] % 32 != 0 and r['idx'] != list(range(r['N']))


def _fwd_routes(r):
    want, _ = predicted_routes(r['B'], r['T'], r['Lq'], r['heads'], r['predictor'])
    return tuple(sorted(n for n in want if n in FWD_LABELS))


def _video_pass_labels(r):
    """launches of ONE feature-encoder application over T clips (forward.hip enc_fwd)"""
    return ['convblock_fwd'] + (['attn_block_fwd'] if r['heads'] == 8 and r['T'] <= 128 else ['attn_fwd', 'attn_out_fwd'])


def test_the_cases_cross_every_boundary_the_issue_names():
    rows = [p.values[0] for p in CASES]
    assert {r['T'] for r in rows} == {24, 117, 128, 160, 256, 300, 1024}
    assert {r['Lq'] for r in rows} == {9, 32, 33, 70}
    assert {r['heads'] for r in rows} == {8, 4, 1}
    assert any(r['predictor'] == 'rnn' and r['B'] <= 80 for r in rows) and any(r['predictor'] == 'rnn' and r['B'] == 96 for r in rows)
    assert any(r['N'] == 1 and r['B'] == 64 for r in rows) and any(r['N'] == 64 and r['B'] == 1 for r in rows)
    assert any(r['N'] != r['B'] and len(set(r['idx'])) < min(r['N'], r['B']) for r in rows)            # repeated AND unused videos
    assert any(r['bf16'] for r in rows) and any(r['word_table'] for r in rows) and any(r['extreme'] for r in rows)
    assert any(r['extreme'] and r['T'] % 32 for r in rows) and any(r['T'] % 32 and 0 in r['idx'] for r in rows)    # off-tile: one clip, and a video that fills T
    # the tolerance gate covers T 117 and 300 alone; whole-tile T and T <= 32 stay bit-exact without exception
    assert {r['T'] for r in rows if off_tile_moved(r)} == {117, 300} and any(r['T'] in (117, 300) and not off_tile_moved(r) for r in rows)
    fold = {(r['T'] <= 128 and r['Lq'] <= 32) for r in rows}
    qfused = {(r['heads'] == 8 and r['Lq'] <= 32) for r in rows}
    assert fold == {True, False} and qfused == {True, False}
    seen = set()
    for r in rows:
        seen |= set(_fwd_routes(r))
    assert seen == set(FWD_LABELS), sorted(set(FWD_LABELS) - seen)


def _setup(r, param_seed=501, batch_seed=502):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg = O.make_cfg(max_pos_len=max(r['T'], r['Lq']), word_size=102, num_heads=r['heads'], predictor=r['predictor'], video_feature_dim=r['Dv'],
                     **({'word_table': True} if r['word_table'] else {}))
    P = O.random_params(cfg, seed=param_seed)
    vb, qb = _videos_and_queries(cfg, r['N'], r['B'], r['T'], r['Lq'], r['Lc'], batch_seed, ragged=r['ragged'], extreme=r['extreme'])
    dv = {k: v.cuda().contiguous() for k, v in vb.items()}
    dq = {k: v.cuda().contiguous() for k, v in qb.items()}
    if r['bf16']:
        dv['vfeats'] = dv['vfeats'].to(torch.bfloat16)
    eng = Engine(cfg)
    flat = flat_from_state_dict(eng, P)
    pad, glove = P.get('embedding_net.word_emb.pad_vec'), P.get('embedding_net.word_emb.glove_vec')
    pg = (None if pad is None else pad.cuda(), None if glove is None else glove.cuda())
    return cfg, P, vb, qb, dv, dq, eng, flat, pg


def _ledger(eng, fn):
    eng.profile_select('*')
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [x['name'] for x in eng.profile_launches()]
    finally:
        eng.profile_select(None)
    return out, names


def _check_ledgers(r, cid, names_enc, names_loc, names_inf):
    """issue item 4: localize = the inference forward of the shape minus vproj_fwd minus one application's encoder launches plus one vmask_gather;
    encode_video = one vproj_fwd, one application's encoder launches, the pack, nothing of the query side or behind the join"""
    vp = _video_pass_labels(r)
    assert 'vproj_fwd' not in names_loc and names_loc.count('vmask_gather') == 1, (cid, names_loc)
    want = Counter(names_inf) - Counter(['vproj_fwd'] + vp) + Counter(['vmask_gather'])
    assert Counter(names_loc) == want, (cid, 'localize', names_loc, 'inference forward', names_inf)
    assert Counter(names_enc) == Counter(['pack', 'vproj_fwd'] + vp), (cid, names_enc)
    assert not [n for n in names_enc if n in ('embed_fwd', 'query_fwd', 'linear_fwd', 'head_fwd', 'vmask_gather') or n.startswith('cq_')], (cid, names_enc)


@pytest.mark.gpu
@pytest.mark.parametrize('r', CASES)
def test_localize_has_the_bits_of_the_inference_forward_on_the_replicated_batch(r, request):
    cid = request.node.callspec.id
    cfg, P, vb, qb, dv, dq, eng, flat, pg = _setup(r)
    N, B, T, Lq, Lc = r['N'], r['B'], r['T'], r['Lq'], r['Lc']
    idx = torch.tensor(r['idx'], dtype=torch.int64)
    want = _fwd_routes(r)
    never = tuple(n for n in FWD_LABELS if n not in want)
    # the workspace bounds of this shape (issue item 6)
    n_loc, n_inf = eng.localize_workspace_floats(B, T, Lq, Lc), eng.inference_workspace_floats(B, T, Lq, Lc)
    n_enc, n_inf_n = eng.encode_workspace_floats(N, T), eng.inference_workspace_floats(N, T, Lq, Lc)
    print('[workspace] %s: localize %d / inference %d floats = %.4f ; encode %d / inference(N) %d = %.4f' % (cid, n_loc, n_inf, n_loc / n_inf, n_enc, n_inf_n, n_enc / n_inf_n))
    assert n_loc <= n_inf + B * T, (cid, n_loc, n_inf)
    assert n_enc < n_inf_n, (cid, n_enc, n_inf_n)
    # encode once, localise B queries
    enc, names_enc = _ledger(eng, lambda: eng.encode_video(flat, dv['vfeats'], dv['v_mask']))
    assert (enc.N, enc.T) == (N, T) and enc.encoding.shape == (N, T, 128)
    loc, names_loc = _ledger(eng, lambda: [t.clone() for t in eng.localize(flat, pg[0], pg[1], enc, r['idx'], dq['word_ids'], dq['char_ids'], dq['q_mask'])])
    si_l, ei_l = eng.extract_index(loc[1], loc[2])
    # the reference: the inference forward on the replicated batch
    didx = idx.cuda()
    rep_f, rep_m = dv['vfeats'][didx].contiguous(), dv['v_mask'][didx].contiguous()
    ref, names_inf = _ledger(eng, lambda: [t.clone() for t in eng.forward(flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], rep_f, rep_m, dq['q_mask'], inference=True)])
    si_r, ei_r = eng.extract_index(ref[1], ref[2])
    check_routes(names_inf, want, never, context=cid + ' (inference forward)')
    check_routes(names_loc, (), never, context=cid + ' (localize)')      # (what it must launch: _check_ledgers, against the inference forward's ledger)
    print('[ledger] %s: encode_video %s ; localize %s' % (cid, names_enc, names_loc))
    _check_ledgers(r, cid, names_enc, names_loc, names_inf)
    padm = rep_m == 0
    if off_tile_moved(r):
        rn, ln = [t.cpu().numpy() for t in ref], [t.cpu().numpy() for t in loc]
        print('[off-tile] %s: elements differing from the inference forward: h_score %d, start %d, end %d of %d' % (
            cid, int((rn[0] != ln[0]).sum()), int((rn[1] != ln[1]).sum()), int((rn[2] != ln[2]).sum()), rn[0].size))
        _gate(cid, ln[0], ln[1], ln[2], rn[0], rn[1], rn[2], padm.cpu().numpy())
    else:
        for nm, a, c in zip(('h_score', 'start_logits', 'end_logits'), ref, loc):
            assert torch.equal(a, c), '%s: %s differs from the inference forward, max |diff| %g' % (cid, nm, float((a - c).abs().max()))
    assert torch.equal(si_l, si_r) and torch.equal(ei_l, ei_r), cid
    assert bool((loc[1][padm] == -1e30).all()) and bool((loc[2][padm] == -1e30).all()) and bool((loc[0][padm] == 0).all()), cid
    # a device index is taken as it is (int64 or int32): same bits
    again = eng.localize(flat, pg[0], pg[1], enc, didx, dq['word_ids'], dq['char_ids'], dq['q_mask'])
    assert all(torch.equal(a, c) for a, c in zip(loc, again)), cid
    # the encoding is the saved path's `venc` of the N videos, bit for bit
    kept = enc.encoding.clone()
    eng.forward(flat, pg[0], pg[1], dv['word_ids'], dv['char_ids'], dv['vfeats'], dv['v_mask'], dv['q_mask'], training=False)
    venc = eng.ws_view('venc', (N, T, 128))
    assert torch.equal(kept, venc), '%s: the encoding differs from the saved venc, max |diff| %g' % (cid, float((kept - venc).abs().max()))


# ------------------------------------------------------------------------------------------------ 4. the ledger, spelled out on three shapes
@pytest.mark.gpu
@pytest.mark.parametrize('T,Lq,heads,predictor', [(128, 9, 8, 'transformer'), (160, 33, 8, 'transformer'), (117, 33, 4, 'rnn')])
def test_ledger_of_encode_video_and_localize(T, Lq, heads, predictor):
    r = dict(N=3, B=5, idx=[0, 2, 2, 0, 1], T=T, Lq=Lq, heads=heads, predictor=predictor, Dv=64, ragged=True, extreme=False, bf16=False, word_table=False, Lc=6)
    cfg, P, vb, qb, dv, dq, eng, flat, pg = _setup(r)
    enc, names_enc = _ledger(eng, lambda: eng.encode_video(flat, dv['vfeats'], dv['v_mask']))
    _, names_loc = _ledger(eng, lambda: eng.localize(flat, pg[0], pg[1], enc, r['idx'], dq['word_ids'], dq['char_ids'], dq['q_mask']))
    didx = torch.tensor(r['idx']).cuda()
    _, names_inf = _ledger(eng, lambda: eng.forward(flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dv['vfeats'][didx].contiguous(),
                                                    dv['v_mask'][didx].contiguous(), dq['q_mask'], inference=True))
    print('[ledger] T %d Lq %d H %d %s\n  inference forward: %s\n  encode_video:      %s\n  localize:          %s' % (T, Lq, heads, predictor, names_inf, names_enc, names_loc))
    _check_ledgers(r, 'T%d' % T, names_enc, names_loc, names_inf)
    vp = _video_pass_labels(r)
    assert names_enc.count('vproj_fwd') == 1 and all(names_enc.count(n) == 1 for n in vp)
    n_app = 3 if predictor == 'transformer' else 1                    # encoder applications a localize call still runs over T clips (+ the query's)
    assert names_loc.count('convblock_fwd') == names_inf.count('convblock_fwd') - 1
    assert names_inf.count('convblock_fwd') >= n_app
    assert names_loc.count('pack') == names_inf.count('pack')


# ------------------------------------------------------------------------------------------------ 5. the reference's numbers
def _gate(name, h, sl, el, rh, rsl, rel, pad):
    """the gates of test_inference_forward_matches_the_reference_goldens: logits 1e-4 * scale, h_score 2e-5, pad positions exact"""
    fin = np.abs(rsl) < 1e29
    scale = max(1.0, float(np.abs(rsl[fin]).max()), float(np.abs(rel[fin]).max()))
    es, ee, eh = float(np.abs(sl - rsl)[fin].max()), float(np.abs(el - rel)[fin].max()), float(np.abs(h - rh).max())
    print('%s: start %.3g end %.3g (gate %.3g), h_score %.3g (gate 2e-5)' % (name, es, ee, 1e-4 * scale, eh))
    assert es < 1e-4 * scale and ee < 1e-4 * scale
    assert eh < 2e-5
    assert np.all(sl[pad] == np.float32(-1e30)) and np.all(el[pad] == np.float32(-1e30)) and np.all(h[pad] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['real_tf', 'long_tf', 'tiny_rnn'])
def test_localize_matches_the_reference_goldens(name):
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg, P, b, z = load_golden(name)
    eng = Engine(cfg)
    flat = flat_from_state_dict(eng, P)
    d = {k: v.cuda().contiguous() for k, v in b.items()}
    B = d['vfeats'].shape[0]
    enc = eng.encode_video(flat, d['vfeats'], d['v_mask'])
    h, sl, el = eng.localize(flat, P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda(), enc, np.arange(B),
                             d['word_ids'], d['char_ids'], d['q_mask'])
    h, sl, el = (t.cpu().numpy() for t in (h, sl, el))
    _gate(name, h, sl, el, z['out.h_score'], z['out.start_logits'], z['out.end_logits'], b['v_mask'].numpy() == 0)
    si, ei = eng.extract_index(torch.from_numpy(sl).cuda(), torch.from_numpy(el).cuda())
    assert np.array_equal(si.cpu().numpy(), z['out.start_index']) and np.array_equal(ei.cpu().numpy(), z['out.end_index'])


@pytest.mark.gpu
@pytest.mark.parametrize('predictor,T,Lq', [('transformer', 64, 9), ('transformer', 160, 33), ('rnn', 64, 9)])
def test_many_queries_per_video_match_the_oracle_restatement(predictor, T, Lq):
    r = dict(N=3, B=7, idx=[0, 0, 2, 1, 0, 2, 2], T=T, Lq=Lq, heads=8, predictor=predictor, Dv=64, ragged=True, extreme=False, bf16=False, word_table=False, Lc=6)
    cfg, P, vb, qb, dv, dq, eng, flat, pg = _setup(r, param_seed=511, batch_seed=512)
    with torch.no_grad():
        rh, rsl, rel, renc = oracle_localize(P, cfg, vb['vfeats'], vb['v_mask'], r['idx'], qb['word_ids'], qb['char_ids'], qb['q_mask'])
    enc = eng.encode_video(flat, dv['vfeats'], dv['v_mask'])
    h, sl, el = eng.localize(flat, pg[0], pg[1], enc, r['idx'], dq['word_ids'], dq['char_ids'], dq['q_mask'])
    e_enc = float((enc.encoding.cpu() - renc).abs().max())
    print('%s T %d Lq %d: encoding differs from the oracle\'s by %.3g' % (predictor, T, Lq, e_enc))
    assert e_enc < 1e-4 * max(1.0, float(renc.abs().max()))
    pad = vb['v_mask'][r['idx']].numpy() == 0
    _gate('%s T %d' % (predictor, T), h.cpu().numpy(), sl.cpu().numpy(), el.cpu().numpy(), rh.numpy(), rsl.numpy(), rel.numpy(), pad)
    si, ei = eng.extract_index(sl, el)
    osi, oei = O.extract_index(rsl, rel)
    assert torch.equal(si.cpu(), osi) and torch.equal(ei.cpu(), oei)


# ------------------------------------------------------------------------------------------------ 6. workspace
@pytest.mark.gpu
def test_workspace_bounds_for_every_shape_of_the_bit_equality_cases():
    """localize <= the inference plan of (B, T, Lq, Lc) + B T floats (the gathered mask is the only growth: the inference plan already reuses the
    video encoder's output slot for the second predictor pass); encode < the inference plan of N samples (encoder scratch and packs only).
    What the feature saves in memory is outside the workspace: the (B, T, Dv) replicated feature block is never built."""
    from vslnet_amd.engine import Engine
    for p in CASES:
        r = p.values[0]
        eng = Engine(O.make_cfg(max_pos_len=max(r['T'], r['Lq']), word_size=102, num_heads=r['heads'], predictor=r['predictor'], video_feature_dim=r['Dv'],
                                **({'word_table': True} if r['word_table'] else {})))
        N, B, T, Lq, Lc = r['N'], r['B'], r['T'], r['Lq'], r['Lc']
        n_loc, n_inf = eng.localize_workspace_floats(B, T, Lq, Lc), eng.inference_workspace_floats(B, T, Lq, Lc)
        n_enc, n_inf_n = eng.encode_workspace_floats(N, T), eng.inference_workspace_floats(N, T, Lq, Lc)
        print('[workspace] %-34s localize / inference = %.4f   encode / inference(N) = %.4f' % (p.id, n_loc / n_inf, n_enc / n_inf_n))
        assert n_loc <= n_inf + B * T, (p.id, n_loc, n_inf)
        assert n_enc < n_inf_n, (p.id, n_enc, n_inf_n)
    # the shapes of tools/localize_rate.py
    for predictor, Dv, B, T, Lq in (('transformer', 1024, 64, 128, 20), ('transformer', 4096, 32, 256, 20), ('transformer', 1024, 64, 1024, 20), ('rnn', 1024, 16, 128, 20)):
        eng = Engine(O.make_cfg(max_pos_len=T, word_size=102, predictor=predictor, video_feature_dim=Dv))
        n_loc, n_inf, n_enc = eng.localize_workspace_floats(B, T, Lq, 10), eng.inference_workspace_floats(B, T, Lq, 10), eng.encode_workspace_floats(B, T)
        print('[workspace] %s Dv %d B %d T %d: localize / inference = %.4f   encode(B videos) / inference = %.4f   replicated features not built: %.1f MiB'
              % (predictor, Dv, B, T, n_loc / n_inf, n_enc / n_inf, B * T * Dv * 4 / 2 ** 20))
        assert n_loc <= n_inf + B * T and n_enc < n_inf


# ------------------------------------------------------------------------------------------------ 7. misuse fails loudly
def _module(cfg, P):
    from model.VSLNet import VSLNet
    m = VSLNet(cfg, np.zeros((cfg.word_size - 2, cfg.word_dim), np.float32))
    m.load_state_dict(P, strict=True)
    return m


@pytest.mark.gpu
def test_module_misuse_raises_with_the_cause_in_the_message():
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=96, word_size=102)
    P = O.random_params(cfg, seed=521)
    vb, qb = _videos_and_queries(cfg, 3, 5, 64, 9, 6, seed=522)
    dv = {k: v.cuda() for k, v in vb.items()}
    dq = {k: v.cuda() for k, v in qb.items()}
    idx = [0, 2, 2, 1, 0]
    q = (dq['word_ids'], dq['char_ids'], dq['q_mask'])
    m = _module(cfg, P).to('cuda')
    m.eval()
    with pytest.raises(RuntimeError, match='grad is enabled'):
        m.encode_video(dv['vfeats'], dv['v_mask'])
    with torch.no_grad():
        enc = m.encode_video(dv['vfeats'], dv['v_mask'])
        out = [t.clone() for t in m.localize(enc, idx, *q)]
        ref = m(dq['word_ids'], dq['char_ids'], dv['vfeats'][idx], dv['v_mask'][idx], dq['q_mask'])
        assert all(torch.equal(a, c) for a, c in zip(out, ref))
        assert all(t.grad_fn is None and not t.requires_grad for t in out)
    with pytest.raises(RuntimeError, match='grad is enabled'):
        m.localize(enc, idx, *q)
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match='train mode'):
        m.localize(enc, idx, *q)
    m.eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match='stale'):                                  # train() may have changed the parameters
            m.localize(enc, idx, *q)
        enc = m.encode_video(dv['vfeats'], dv['v_mask'])
        assert all(torch.equal(a, c) for a, c in zip(out, m.localize(enc, idx, *q, T=64)))
        with pytest.raises(ValueError, match='T=64, not T=96'):                         # an encoding belongs to its padded T
            m.localize(enc, idx, *q, T=96)
        with pytest.raises(ValueError, match='out of range'):
            m.localize(enc, [0, 3, 2, 1, 0], *q)
        with pytest.raises(ValueError, match='out of range'):
            m.localize(enc, torch.tensor([0, -1, 2, 1, 0]), *q)
        other = _module(cfg, P).to('cuda').eval()
        with pytest.raises(ValueError, match='another module'):
            other.localize(enc, idx, *q)
        m.load_state_dict(P, strict=True)
        with pytest.raises(ValueError, match='stale'):
            m.localize(enc, idx, *q)
        with pytest.raises(ValueError, match='N >= 1'):
            m.encode_video(dv['vfeats'][:0], dv['v_mask'][:0])


@pytest.mark.gpu
def test_engine_refuses_backward_and_taps_after_localize_and_an_empty_call():
    import ctypes as C
    from vslnet_amd.engine import VslError, vsl_encode_io, vsl_io, vsl_localize_io
    r = dict(N=3, B=4, idx=[0, 2, 2, 1], T=96, Lq=9, heads=8, predictor='transformer', Dv=64, ragged=True, extreme=False, bf16=False, word_table=False, Lc=6)
    cfg, P, vb, qb, dv, dq, eng, flat, pg = _setup(r)
    assert eng.has_shared_video
    # a saved-path forward on the replicated batch, then localize in the same (shared) workspace
    didx = torch.tensor(r['idx']).cuda()
    args = (flat, pg[0], pg[1], dq['word_ids'], dq['char_ids'], dv['vfeats'][didx].contiguous(), dv['v_mask'][didx].contiguous(), dq['q_mask'])
    h, sl, el = eng.forward(*args, training=False)
    io = vsl_io()
    C.memmove(C.byref(io), C.byref(eng._last), C.sizeof(vsl_io))
    ws = eng._last_ws
    enc = eng.encode_video(flat, dv['vfeats'], dv['v_mask'])
    for what in ('encode_video', 'localize'):
        if what == 'localize':
            eng.localize(flat, pg[0], pg[1], enc, r['idx'], dq['word_ids'], dq['char_ids'], dq['q_mask'])
        with pytest.raises(VslError, match='saved nothing'):
            eng.backward(torch.zeros_like(h), torch.zeros_like(sl), torch.zeros_like(el), eng.new_flat())
        with pytest.raises(VslError, match='saves nothing'):
            eng.ws_view('gated', (r['B'], r['T'], 128))
        # the library on its own: the saved-path io of before, whose workspace the call has overwritten
        assert eng._ws.data_ptr() == ws.data_ptr()
        z, g = torch.zeros_like(sl), eng.new_flat()
        io.d_start_logits, io.d_end_logits, io.grads = z.data_ptr(), z.data_ptr(), g.data_ptr()
        assert eng.lib.vsl_backward(eng.h, C.byref(io), None) != 0 and b'saved nothing' in eng.lib.vsl_last_error()
        assert eng.lib.vsl_workspace_offset(eng.h, r['B'], r['T'], r['Lq'], r['Lc'], b'gated') == -2 and b'saved nothing' in eng.lib.vsl_last_error()
    # empty and incomplete calls
    e = vsl_encode_io()
    e.N, e.T = 0, r['T']
    e.params, e.video_features, e.v_mask, e.video_encoding, e.workspace = (flat.data_ptr(), dv['vfeats'].data_ptr(), dv['v_mask'].data_ptr(),
                                                                             enc.encoding.data_ptr(), eng._ws.data_ptr())
    assert eng.lib.vsl_encode_video(eng.h, C.byref(e), None) != 0 and b'N=0' in eng.lib.vsl_last_error()
    n = C.c_int64()
    assert eng.lib.vsl_encode_workspace_floats(eng.h, 0, r['T'], C.byref(n)) != 0 and b'N=0' in eng.lib.vsl_last_error()
    lo = vsl_localize_io()
    lo.B, lo.T, lo.Lq, lo.Lc, lo.N = 0, r['T'], r['Lq'], r['Lc'], r['N']
    assert eng.lib.vsl_localize(eng.h, C.byref(lo), None) != 0 and b'B=0' in eng.lib.vsl_last_error()
    lo.B = r['B']
    assert eng.lib.vsl_localize(eng.h, C.byref(lo), None) != 0 and b'video_encoding is NULL' in eng.lib.vsl_last_error()
    lo.video_encoding = enc.encoding.data_ptr()
    assert eng.lib.vsl_localize(eng.h, C.byref(lo), None) != 0 and b'video_index is NULL' in eng.lib.vsl_last_error()
    lo.video_index = didx.to(torch.int32).data_ptr()
    assert eng.lib.vsl_localize(eng.h, C.byref(lo), None) != 0 and b'v_mask is NULL' in eng.lib.vsl_last_error()
    lo.v_mask, lo.N = dv['v_mask'].data_ptr(), 0
    assert eng.lib.vsl_localize(eng.h, C.byref(lo), None) != 0 and b'N=0' in eng.lib.vsl_last_error()
    with pytest.raises(ValueError, match='N >= 1'):
        eng.encode_video(flat, dv['vfeats'][:0], dv['v_mask'][:0])
    # an older library (no such symbols): both methods raise
    eng.has_shared_video = False
    with pytest.raises(VslError, match='no shared-video entry points'):
        eng.encode_video(flat, dv['vfeats'], dv['v_mask'])
    with pytest.raises(VslError, match='no shared-video entry points'):
        eng.localize(flat, pg[0], pg[1], enc, r['idx'], dq['word_ids'], dq['char_ids'], dq['q_mask'])
    eng.has_shared_video = True
    # the saved path again: backward and taps work
    eng.forward(*args, training=False)
    assert eng.ws_view('gated', (r['B'], r['T'], 128)).shape == (r['B'], r['T'], 128)


@pytest.mark.gpu
@pytest.mark.parametrize('predictor', ['transformer', 'rnn'])
def test_a_training_step_after_localize_in_the_same_engine_meets_the_oracle(predictor, monkeypatch):
    """The shared workspace is handed back cleanly: check_training_against_oracle builds its own engine, so the engine it gets has already
    encoded three videos and localised five queries of the same T / Lq in the workspace the step then trains in."""
    from vslnet_amd import engine as E
    B, T, Lq, Lc = 4, 96, 9, 6
    made = []

    class Used(E.Engine):
        def __init__(self, cfg, *a, **k):
            super().__init__(cfg, *a, **k)
            P = O.random_params(cfg, seed=531)
            flat = E.flat_from_state_dict(self, P)
            vb, qb = _videos_and_queries(cfg, 3, 5, T, Lq, Lc, seed=532)
            enc = self.encode_video(flat, vb['vfeats'].cuda(), vb['v_mask'].cuda())
            self.localize(flat, P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda(), enc, [0, 2, 2, 1, 0],
                          qb['word_ids'].cuda(), qb['char_ids'].cuda(), qb['q_mask'].cuda())
            torch.cuda.synchronize()
            made.append(self)
    monkeypatch.setattr(E, 'Engine', Used)
    out = check_training_against_oracle(B, T, Lq, Lc, cfg=dict(predictor=predictor, video_feature_dim=64), lazy=True, context='after localize (%s)' % predictor)
    assert len(made) == 1 and out.eng is made[0]


# ------------------------------------------------------------------------------------------------ 8. the evaluation loop
def _shared_dataset(configs, n_videos=5, per_video=4, seed=7):
    """records in the reference's format with SEVERAL records per video (data.synthetic_dataset makes one video per record), ragged video lengths"""
    from vslnet_amd.runner import index_to_time
    rs = np.random.RandomState(seed)
    dv, tmax = configs.video_feature_dim, configs.max_pos_len
    feats, recs = {}, []
    for v in range(n_videos):
        L = tmax if v == 1 else int(rs.randint(tmax // 3, tmax))
        feats['v%02d' % v] = rs.randn(L, dv).astype(np.float32)
    order = [v for v in range(n_videos) for _ in range(per_video)]
    rs.shuffle(order)
    for v in order:
        L = feats['v%02d' % v].shape[0]
        s = int(rs.randint(0, L - 2))
        e = int(min(L - 1, s + rs.randint(1, max(2, L // 3))))
        dur = float(L) * 1.5
        w = [int(x) for x in rs.randint(2, configs.word_size, size=int(rs.randint(3, 9)))]
        c = [[2 + (wi * 7 + k) % (configs.char_size - 2) for k in range(1 + wi % 6)] for wi in w]
        st, et = index_to_time(s, e, L, dur)
        recs.append({'sample_id': len(recs), 'vid': 'v%02d' % v, 's_time': float(st), 'e_time': float(et), 'duration': dur,
                     'words': ['w%d' % x for x in w], 's_ind': s, 'e_ind': e, 'v_len': L, 'w_ids': w, 'c_ids': c})
    return recs, feats


@pytest.mark.gpu
def test_eval_test_shared_returns_the_metrics_of_the_loop_padded_to_tmax():
    from model.VSLNet import VSLNet
    from vslnet_amd.data import ResidentSplit
    from vslnet_amd.runner import calculate_iou, eval_test_shared, index_to_time, summarise
    from vslnet_amd.synthetic import make_configs
    configs = make_configs(video_feature_dim=64, max_pos_len=96, word_size=200, char_size=30, batch_size=6, drop_rate=0.2)      # (Tmax on the row tile: exact bits)
    recs, feats = _shared_dataset(configs)
    torch.manual_seed(9)
    m = VSLNet(configs, np.random.RandomState(3).randn(configs.word_size - 2, configs.word_dim).astype(np.float32) * 0.3).to('cuda').eval()
    split = ResidentSplit(recs, feats, configs, 'cuda', train=False)
    assert split.feats.shape[0] == 5 and len(recs) == 20 and split.feats.shape[1] == 96
    got = eval_test_shared(m, split, 'cuda', epoch=1, global_step=1, videos_per_call=2)
    # the same loop written out with the module's forward on replicated features at T = Tmax
    tmax, ious = split.feats.shape[1], []
    with torch.no_grad():
        for a in range(0, len(recs), configs.batch_size):
            idx = np.arange(a, min(len(recs), a + configs.batch_size))
            idx_dev = torch.from_numpy(idx).cuda()
            Lq, Lc = int(split.nwords[idx].max()), int(split.nchars[idx].max())
            word_ids, char_ids = split.d_words[idx_dev][:, :Lq].contiguous(), split.d_chars[idx_dev][:, :Lq, :Lc].contiguous()
            vf = split.feats[:, :tmax][split.d_vid[idx_dev]]
            v_mask = (torch.arange(tmax, device='cuda')[None, :] < split.d_lens[idx_dev][:, None]).float()
            _, sl, el = m(word_ids, char_ids, vf, v_mask, (word_ids != 0).float())
            si, ei = m.extract_index(sl, el)
            for i, s_, e_ in zip(idx, si.cpu().numpy(), ei.cpu().numpy()):
                st, et = index_to_time(int(s_), int(e_), recs[i]['v_len'], recs[i]['duration'])
                ious.append(calculate_iou([st, et], [recs[i]['s_time'], recs[i]['e_time']]))
    want = summarise(ious, 1, 1)
    assert got == want, (got, want)
    # the handle of the split is a handle like any other: stale after train()
    with torch.no_grad():
        enc = split.encode(m, videos_per_call=3)
        assert enc.encoding.shape == (5, 96, 128) and enc.N == 5 and enc.T == 96
        m.train()
        m.eval()
        with pytest.raises(ValueError, match='stale'):
            m.localize(enc, [0], split.d_words[:1, :4].contiguous(), split.d_chars[:1, :4, :4].contiguous(), (split.d_words[:1, :4] != 0).float())
