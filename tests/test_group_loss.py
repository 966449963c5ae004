"""The video ranking loss on the device: vsl_group_loss (k_group_loss_a + k_group_loss_c), Engine.group_loss, VSLNet.compute_video_ranking_loss and a
training step through ResidentSplit.shards(negatives=n).

The specification is vslnet_amd.spans.group_loss_reference (checked on the CPU against autograd in tests/test_group_loss_spec.py).  What is exact is
compared for equality: the relevance (the device's additions, pair_relevance_reference(fp32_order=True)), the hits, the zero rows of the span seeds, where
the rank gradient may be non-zero, and -- with every group of size one -- vsl_loss' own bits.  The loss values and seeds are fp32 expf / logf
against float64; their gate is REL_BOUND below."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vslnet_oracle as O
from tests.test_group_loss_spec import spec_case
from vslnet_amd.spans import group_loss_reference, pair_relevance_reference

pytestmark = pytest.mark.gpu

# Largest error of a loss value or a seed tensor against the float64 specification, relative to the tensor's largest magnitude, over every case of
# test_against_the_specification: MEASURED_REL on an MI355X (ROCm 7 hipcc -O3); the gate is 4 x that (compiler and libm revisions).
MEASURED_REL = 9.2e-7        # (ragged-T33, mean, tau 0.05: the rank gradient alone; the largest loss value: 7.8e-7, G1-of-3 max tau 0.05)
REL_BOUND = 4 * MEASURED_REL


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max())
    return float(np.abs(got - want).max()) / scale if scale > 0 else float(np.abs(got).max())


_ENGINE = {}


def engine():
    """one tiny engine for every test of the file that needs a handle"""
    if 'eng' not in _ENGINE:
        from vslnet_amd.engine import Engine, flat_from_state_dict
        cfg = O.make_cfg(video_feature_dim=64, max_pos_len=288, word_size=52, predictor='transformer', drop_rate=0.0)
        P = O.random_params(cfg, seed=5)
        eng = Engine(cfg)
        _ENGINE.update(eng=eng, cfg=cfg, P=P, flat=flat_from_state_dict(eng, P), pad=P['embedding_net.word_emb.pad_vec'].cuda(),
                       glove=P['embedding_net.word_emb.glove_vec'].cuda())
    return _ENGINE['eng']


def cuda(c):
    return {k: torch.from_numpy(v).cuda() for k, v in c.items()}


def run_case(c, mode, tau, w=(1.0, 5.0, 0.7), labels=True, **kw):
    eng, d = engine(), cuda(c)
    out = eng.group_loss(d['s_lab'] if labels else None, d['e_lab'] if labels else None, d['h_lab'] if labels else None, d['gs'], d['pos'],
                         w[0], w[1], w[2], tau, mode, scores=d['h'], start_logits=d['sl'], end_logits=d['el'], v_mask=d['mask'], **kw)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


# ------------------------------------------------------------------------------------------------ one definition
@pytest.mark.parametrize('w_rank', [0.0, 1.0])
@pytest.mark.parametrize('B,T', [(5, 7), (5, 33), (3, 257)])
def test_groups_of_one_are_vsl_loss_bit_for_bit(B, T, w_rank):
    eng = engine()
    E = _ENGINE
    d = {k: v.cuda().contiguous() for k, v in O.synthetic_batch(E['cfg'], B=B, T=T, Lq=7, Lc=6, seed=6 + T, ragged=True).items()}
    h, sl, el = eng.forward(E['flat'], E['pad'], E['glove'], d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], training=True, seed=9)
    want = [t.clone() for t in eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0, inv_batch=1.0 / B, lazy=False)]
    gs, pos = torch.arange(B + 1, dtype=torch.int32).cuda(), torch.arange(B, dtype=torch.int32).cuda()
    for mode in ('max', 'mean'):
        # on the last forward's outputs, like Engine.loss
        losses, hits, rel, d_h, d_sl, d_el = eng.group_loss(d['s_labels'], d['e_labels'], d['h_labels'], gs, pos, 1.0, 5.0, w_rank, 0.05, mode, inv_pos=1.0 / B)
        torch.cuda.synchronize()
        assert torch.equal(losses[[0, 1, 4]], want[0][[0, 1, 3]]), (losses, want[0])
        assert float(losses[2]) == 0.0 and int(hits) == B                      # l_g = 0 in a group of one
        assert abs(float(losses[3]) - float(want[0][2])) <= 1e-6 * abs(float(want[0][2]))      # (+ w_rank * 0; the weighted sum may contract differently)
        for got, ref, nm in ((d_h, want[1], 'd_h'), (d_sl, want[2], 'd_sl'), (d_el, want[3], 'd_el')):
            assert bool((got == ref).all()), (nm, mode, float((got - ref).abs().max()))
        assert np.array_equal(rel.cpu().numpy(), pair_relevance_reference(h.cpu().numpy(), d['v_mask'].cpu().numpy(), mode, fp32_order=True))


# ------------------------------------------------------------------------------------------------ against the specification
CASES = [('ragged-T%d' % T, dict(T=T, seed=T)) for T in (1, 33, 65, 257)] + [('one-group-of-70', dict(T=8, sizes=(70,), seed=4)),
                                                                              ('G1-of-3', dict(T=33, sizes=(3,), seed=5))]


@pytest.mark.parametrize('mode', ['max', 'mean'])
@pytest.mark.parametrize('tau', [1.0, 0.05])
@pytest.mark.parametrize('name,kw', CASES, ids=[n for n, _ in CASES])
def test_against_the_specification(name, kw, tau, mode):
    c = spec_case(**kw)
    B, T = c['h'].shape
    losses, hits, rel, d_h, d_sl, d_el = run_case(c, mode, tau)
    want = group_loss_reference(c['h'], c['sl'], c['el'], c['mask'], c['s_lab'], c['e_lab'], c['h_lab'], c['gs'], c['pos'], 1.0, 5.0, 0.7, tau, mode)
    # exact
    assert rel.tobytes() == pair_relevance_reference(c['h'], c['mask'], mode, fp32_order=True).tobytes()
    assert int(hits) == want.hits
    is_pos = np.zeros(B, dtype=bool)
    is_pos[c['pos']] = True
    assert not d_sl[~is_pos].any() and not d_el[~is_pos].any()
    assert float(losses[4]) == float(c['mask'].sum())
    # the rank gradient alone (no labels, weights 0): zero off the argmax / off the mask, exactly
    l0, hits0, _, r_h, r_sl, r_el = run_case(c, mode, tau, w=(0.0, 0.0, 0.7), labels=False)
    assert not r_sl.any() and not r_el.any() and float(l0[0]) == 0.0 and float(l0[1]) == 0.0 and int(hits0) == want.hits
    assert not r_h[c['mask'] == 0].any()
    if mode == 'max':
        first = np.array([np.flatnonzero((c['mask'][b] != 0) & (c['h'][b] == rel[b]))[0] if np.isfinite(rel[b]) else 0 for b in range(B)])
        off = np.ones((B, T), dtype=bool)
        off[np.arange(B), first] = False
        assert not r_h[off].any()
    # fp32 against float64
    figures = {'loc': rel_err(losses[0], want.losses[0]), 'hl': rel_err(losses[1], want.losses[1]), 'rank': rel_err(losses[2], want.losses[2]),
               'total': rel_err(losses[3], want.losses[3]), 'd_h': rel_err(d_h, want.d_h), 'd_sl': rel_err(d_sl, want.d_sl), 'd_el': rel_err(d_el, want.d_el),
               'rank_d_h': rel_err(r_h, group_loss_reference(c['h'], c['sl'], c['el'], c['mask'], None, None, None, c['gs'], c['pos'], 0.0, 0.0, 0.7, tau, mode).d_h)}
    print('GROUP_LOSS_FIGURES', name, mode, tau, ' '.join('%s=%.3e' % kv for kv in figures.items()), 'max=%.3e' % max(figures.values()))
    for k, v in figures.items():
        assert v <= REL_BOUND, (k, v, REL_BOUND)


def test_two_calls_give_the_same_bits():
    c = spec_case(T=65, seed=65)
    for mode in ('max', 'mean'):
        a = run_case(c, mode, 0.05)
        b = run_case(c, mode, 0.05)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        lo = run_case(c, mode, 0.05, want_grads=False)                         # the loss values alone: the same bits, no seeds
        assert lo[0].tobytes() == a[0].tobytes() and int(lo[1]) == int(a[1]) and lo[3] is None


def test_a_caller_supplied_mask_sum_is_used():
    c = spec_case(T=33, seed=33)
    losses, _, _, d_h, _, _ = run_case(c, 'max', 0.1, mask_sum=500.0)
    want = group_loss_reference(c['h'], c['sl'], c['el'], c['mask'], c['s_lab'], c['e_lab'], c['h_lab'], c['gs'], c['pos'], 1.0, 5.0, 0.7, 0.1, 'max', mask_sum=500.0)
    assert float(losses[4]) == 500.0
    assert rel_err(losses[1], want.losses[1]) <= REL_BOUND and rel_err(d_h, want.d_h) <= REL_BOUND


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_is_named_and_launches_nothing():
    from vslnet_amd.engine import vsl_group_loss_io
    eng = engine()
    c = cuda(spec_case(T=7, seed=1))
    B, T, G = 12, 7, 4
    keep = [torch.zeros(10 * B + 8).cuda(), torch.zeros(5).cuda(), torch.zeros(3, B, T).cuda()]
    p = lambda t: C.c_void_p(t.data_ptr())

    def good():
        l = vsl_group_loss_io()
        l.B, l.T, l.G = B, T, G
        l.h_score, l.start_logits, l.end_logits, l.v_mask = p(c['h']), p(c['sl']), p(c['el']), p(c['mask'])
        l.start_labels, l.end_labels, l.h_labels = p(c['s_lab']), p(c['e_lab']), p(c['h_lab'])
        l.group_start, l.positive = p(c['gs']), p(c['pos'])
        l.w_loc, l.w_highlight, l.w_rank, l.inv_pos, l.inv_groups, l.mask_sum, l.inv_temperature, l.relevance = 1.0, 5.0, 1.0, 0.25, 0.25, 0.0, 10.0, 0
        l.losses, l.scratch = p(keep[1]), p(keep[0])
        l.d_h_score, l.d_start_logits, l.d_end_logits = p(keep[2][0]), p(keep[2][1]), p(keep[2][2])
        return l

    bad = [(dict(h_score=None), 'h_score'), (dict(start_logits=None), 'start_logits'), (dict(end_logits=None), 'end_logits'), (dict(v_mask=None), 'v_mask'),
           (dict(group_start=None), 'group_start'), (dict(positive=None), 'positive'), (dict(losses=None), 'losses'), (dict(scratch=None), 'scratch'),
           (dict(B=0), 'B=0'), (dict(G=0), 'G=0'), (dict(T=0), 'T=0'), (dict(G=B + 1), 'G=13'), (dict(T=4097), 'T=4097'),
           (dict(d_h_score=None), 'all set or all null'), (dict(d_end_logits=None), 'all set or all null'),
           (dict(inv_temperature=0.0), 'inv_temperature'), (dict(inv_temperature=-1.0), 'inv_temperature'),
           (dict(relevance=2), 'relevance=2'), (dict(relevance=-1), 'relevance=-1'),
           (dict(start_labels=None, end_labels=None), 'w_loc'), (dict(start_labels=None), 'both'), (dict(h_labels=None), 'w_highlight')]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    eng.profile_select('*')
    try:
        for change, word in bad:
            l = good()
            for k, v in change.items():
                setattr(l, k, v)
            assert eng.lib.vsl_group_loss(eng.h, C.byref(l), stream) != 0, change
            assert word in eng.lib.vsl_last_error().decode(), (change, eng.lib.vsl_last_error())
        assert eng.lib.vsl_group_loss(None, C.byref(good()), stream) != 0 and 'null argument' in eng.lib.vsl_last_error().decode()
        assert eng.profile_launches() == []                                    # nothing was launched
        assert eng.lib.vsl_group_loss(eng.h, C.byref(good()), stream) == 0
        torch.cuda.synchronize()
        assert [r['name'] for r in eng.profile_launches()] == ['group_loss_a', 'group_loss_c']
    finally:
        eng.profile_select(None)
    with pytest.raises(ValueError, match="'max' or 'mean'"):
        eng.group_loss(None, None, None, c['gs'], c['pos'], 0.0, 0.0, relevance='sum', scores=c['h'], start_logits=c['sl'], end_logits=c['el'], v_mask=c['mask'])


# ------------------------------------------------------------------------------------------------ the module
def test_module_ranking_loss_back_propagates_the_kernels_seed():
    from vslnet_amd.model.VSLNet import VSLNet
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=64, word_size=52, predictor='transformer', drop_rate=0.0)
    torch.manual_seed(3)
    model = VSLNet(cfg, np.zeros((cfg.word_size - 2, cfg.word_dim), np.float32)).cuda()
    c = cuda(spec_case(T=33, seed=33))
    for mode in ('max', 'mean'):
        h = c['h'].clone().requires_grad_(True)
        loss = model.compute_video_ranking_loss(h, c['mask'], c['gs'], c['pos'], temperature=0.05, relevance=mode)
        (3.0 * loss).backward()
        want = model._engine.group_loss(None, None, None, c['gs'], c['pos'], 0.0, 0.0, 1.0, 0.05, mode, scores=c['h'], start_logits=c['h'], end_logits=c['h'],
                                        v_mask=c['mask'])
        torch.cuda.synchronize()
        assert float(loss) == float(want[0][2]) > 0
        assert torch.equal(h.grad, 3.0 * want[3]) and bool(h.grad.any())


# ------------------------------------------------------------------------------------------------ end to end
def _train_30_steps():
    from types import SimpleNamespace
    from vslnet_amd import data
    from vslnet_amd.dp import FlatAdamW
    from vslnet_amd.engine import Engine, flat_from_state_dict
    cfg = O.make_cfg(video_feature_dim=64, max_pos_len=32, word_size=52, char_size=30, predictor='transformer', drop_rate=0.0)
    dcfg = SimpleNamespace(video_feature_dim=64, max_pos_len=32, word_dim=300, batch_size=16)
    dataset, feats = data.synthetic_dataset(dcfg, n_train=4, n_test=1, n_words=52, seed=2)
    recs = dataset['train_set']
    assert len({r['w_ids'][0] for r in recs}) == 4                             # four different events: no false negative among the in-batch videos
    split = data.ResidentSplit(recs, feats, dcfg, 'cuda', train=True, generator=torch.Generator().manual_seed(5))
    batch, = list(split.shards(negatives=3))                                   # P = 4 queries, n = 3, 4 videos: groups of 4 rows
    assert batch['group_start'].tolist() == [0, 4, 8, 12, 16] and batch['vfeats'].shape[0] == 4 and batch['vfeats'].shape[1] <= 33
    P = O.random_params(cfg, seed=5)
    eng = Engine(cfg)
    flat = flat_from_state_dict(eng, P)
    pad, glove = P['embedding_net.word_emb.pad_vec'].cuda(), P['embedding_net.word_emb.glove_vec'].cuda()
    opt = FlatAdamW(flat, eng.layout, lr=1e-3, num_train_steps=30, clip_norm=1.0, engine=eng)
    grads, q_mask = eng.new_flat(), (batch['word_ids'] != 0).float()
    mask_sum = float(sum(int(x) for x in batch['lens_global']))
    trace = []
    for step in range(30):
        eng.forward_shared(flat, pad, glove, batch['word_ids'], batch['char_ids'], batch['vfeats'], batch['video_v_mask'], q_mask, batch['video_index'],
                           training=True, seed=step)
        losses, hits, _, *seeds = eng.group_loss(batch['s_labels'], batch['e_labels'], batch['h_labels'], batch['group_start'], batch['positive'], 1.0, 5.0,
                                                 1.0, 0.1, 'max', inv_pos=0.25, inv_groups=0.25, mask_sum=mask_sum)
        eng.backward(*seeds, grads, fused_step=opt.fused_step())
        trace.append((losses.clone(), hits.clone()))
    torch.cuda.synchronize()
    return [(l.cpu().numpy(), int(h)) for l, h in trace], flat.clone()


def test_thirty_steps_on_one_sampler_batch_learn_to_rank_and_repeat_bit_for_bit():
    a, flat_a = _train_30_steps()
    b, flat_b = _train_30_steps()
    print('GROUP_LOSS_E2E rank', ' '.join('%.4f' % l[2] for l, _ in a), '| hits', ' '.join(str(h) for _, h in a))
    assert all(np.isfinite(l).all() for l, _ in a)
    assert a[-1][0][2] < a[0][0][2]                                            # the rank term falls below its value at step 1
    assert a[-1][1] == 4                                                       # every query's own video ranks first
    assert torch.equal(flat_a, flat_b) and all(x[0].tobytes() == y[0].tobytes() and x[1] == y[1] for x, y in zip(a, b))
