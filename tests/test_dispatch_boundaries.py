"""Training-mode parity at every kernel dispatch boundary.

The library picks its kernels by shape (attention forward fused with the span heads or not, the attention backward's element hashes,
key-pair hashes, dQ slabs and query-major dQ, the fused QKV backward, the sample-local query branch, the CQ column fold, the inline loss
seeds, the one-launch rnn head or its chunked LSTMs).  Each row below runs one training step (drop_rate 0.2, the production loss sequence
unless it says otherwise) against the oracle on the HIP path's own dropout masks (tests/helpers.py: check_training_against_oracle) AND
states which launches the step must take: the labels it lists must appear in the step's launch ledger, every other label of ROUTE_LABELS
must not.  The expectations come from the dispatch predicates (predicted_routes mirrors them; a CPU test keeps the table and the mirror
in step), so a moved threshold fails by name instead of drifting onto another route.  A training-mode random sweep covers the shapes
nobody picked by hand."""
import numpy as np
import pytest

from tests.helpers import check_training_against_oracle, extreme_ragged

# the ledger labels a row makes a statement about (forward.hip / backward.hip LAUNCH names)
ROUTE_LABELS = ('attn_block_fwd', 'attn_fwd', 'attn_out_fwd', 'head_fwd', 'qkv_bwd', 'cq_col', 'query_fwd', 'query_bwd', 'linear_fwd',
                'rnn_fwd', 'rnn_bwd', 'lstm_fwd', 'lstm_bwd')


def predicted_routes(B, T, Lq, num_heads=8, predictor='transformer', lazy=True):
    """-> (labels the step launches among ROUTE_LABELS, whether the loss seeds are computed inside the heads' backward), from the predicates:
    query_fused_ok (kernels_query.hip), enc_fwd's attention choice and attn_block_fwd_hosts_heads (forward.hip, launch.hpp), cq_col_folds
    (kernels_cq.hip), convblock_bwd_hosts_qkv + attn_bwd_dq_slabs (kernels_enc.hip, kernels_attn_h16.hip), rnn_fused_ok (kernels_lstm.hip) and
    loss_seeds' seeds_inline (backward.hip)."""
    h8 = num_heads == 8
    query_local = h8 and Lq <= 32
    enc_L = [T] + ([] if query_local else [Lq]) + ([T, T] if predictor == 'transformer' else [])      # the encoder applications' lengths
    out = set()
    if h8 and any(L <= 128 for L in enc_L):
        out.add('attn_block_fwd')
    if any(not h8 or L > 128 for L in enc_L):
        out |= {'attn_fwd', 'attn_out_fwd'}
    if predictor == 'rnn' or not (h8 and T <= 128):
        out.add('head_fwd')
    out |= {'query_fwd', 'query_bwd'} if query_local else {'linear_fwd'}
    if not (T <= 128 and Lq <= 32):
        out.add('cq_col')

    def qkv_fused(L):
        Lp = (L + 15) // 16 * 16
        return (L <= 32 or L % 32 == 0) and Lp <= 256
    if not all(qkv_fused(L) for L in enc_L):
        out.add('qkv_bwd')
    if predictor == 'rnn':
        out |= {'rnn_fwd', 'rnn_bwd'} if B <= 80 else {'lstm_fwd', 'lstm_bwd'}
    return out, bool(lazy and T >= 32)


def row(rid, B, T, Lq, want, inline, heads=8, predictor='transformer', Dv=64, word_dim=300, ragged=False, lazy=True):
    return pytest.param(dict(B=B, T=T, Lq=Lq, heads=heads, predictor=predictor, Dv=Dv, word_dim=word_dim, ragged=ragged, lazy=lazy,
                             want=tuple(want.split()), inline=inline), id=rid)


BLK, SPLIT, QL, LIN = 'attn_block_fwd', 'attn_fwd attn_out_fwd', 'query_fwd query_bwd', 'linear_fwd'
ROWS = [
    # ---- video length, 8 heads, Lq 9 (the sample-local query branch): conv-block tiles, attention forward / backward, QKV fusion, loss seeds
    row('T31-under-a-row-tile-loss-seeds-launched', 5, 31, 9, BLK + ' ' + QL, False),
    row('T32-sample-tile-edge-seeds-inline', 3, 32, 9, BLK + ' ' + QL, True),
    row('T33-ragged-row-tiles-extreme', 3, 33, 9, BLK + ' ' + QL + ' qkv_bwd', True, ragged=True),
    row('T96-whole-tiles', 3, 96, 9, BLK + ' ' + QL, True),
    row('T128-last-attn-block-fwd-and-fused-bwd-extreme', 3, 128, 9, BLK + ' ' + QL, True, ragged=True),
    row('T129-first-element-hash-bwd-long', 3, 129, 9, SPLIT + ' head_fwd cq_col qkv_bwd ' + QL, True),
    row('T160-element-hash-whole-tiles', 3, 160, 9, SPLIT + ' head_fwd cq_col ' + QL, True),
    row('T250-one-256-key-block-extreme', 3, 250, 9, SPLIT + ' head_fwd cq_col qkv_bwd ' + QL, True, ragged=True),
    row('T256-last-element-hash', 2, 256, 9, SPLIT + ' head_fwd cq_col ' + QL, True),
    row('T257-first-key-pair-hash-2-dq-slabs', 2, 257, 9, SPLIT + ' head_fwd cq_col qkv_bwd ' + QL, True),
    row('T512-key-pairs-2-dq-slabs', 1, 512, 9, SPLIT + ' head_fwd cq_col qkv_bwd ' + QL, True),
    row('T1024-last-dq-slab-path-4-slabs', 1, 1024, 9, SPLIT + ' head_fwd cq_col qkv_bwd ' + QL, True),
    row('T1025-first-query-major-dq', 1, 1025, 9, SPLIT + ' head_fwd cq_col qkv_bwd ' + QL, True),
    row('T256-Dv4096-configs2-width', 1, 256, 20, SPLIT + ' head_fwd cq_col ' + QL, True, Dv=4096),
    # ---- query length, 8 heads: the sample-local query kernels (Lq <= 32) against the row-tile launches, the CQ column fold, the cq_score layouts
    row('Lq1-one-word-sample-local', 3, 40, 1, BLK + ' qkv_bwd ' + QL, True),
    row('Lq32-last-sample-local', 3, 64, 32, BLK + ' ' + QL, True),
    row('Lq32-last-sample-local-extreme', 3, 48, 32, BLK + ' qkv_bwd ' + QL, True, ragged=True),
    row('Lq33-first-row-tile-query-cq-col', 3, 40, 33, BLK + ' qkv_bwd cq_col ' + LIN, True),
    row('Lq64-last-cq-score-layout-1', 2, 64, 64, BLK + ' cq_col ' + LIN, True),
    row('Lq65-first-cq-score-layout-2', 2, 50, 65, BLK + ' qkv_bwd cq_col ' + LIN, True),
    row('Lq96-last-cq-score-layout-2', 2, 48, 96, BLK + ' qkv_bwd cq_col ' + LIN, True),
    row('Lq97-first-lean-cq-score-layout', 2, 64, 97, BLK + ' qkv_bwd cq_col ' + LIN, True),
    row('wd52-sample-local-152-wide-embedding', 3, 40, 20, BLK + ' qkv_bwd ' + QL, True, word_dim=52),
    row('wd52-fp32-input-linear-Lq40', 3, 56, 40, BLK + ' qkv_bwd cq_col ' + LIN, True, word_dim=52),
] + [
    # ---- 4 and 16 heads (kernels_attn_hd.hip: no L <= 128 fusion, no sample-local query branch)
    r for H in (4, 16) for r in [
        row('H%d-T32-Lq1-single-key' % H, 3, 32, 1, LIN + ' ' + SPLIT + ' head_fwd', True, heads=H),
        row('H%d-T129-Lq33-element-hash-row-tiles' % H, 3, 129, 33, LIN + ' ' + SPLIT + ' head_fwd cq_col qkv_bwd', True, heads=H),
        row('H%d-T256-last-element-hash' % H, 2, 256, 9, LIN + ' ' + SPLIT + ' head_fwd cq_col', True, heads=H),
        row('H%d-T257-first-key-pair-hash' % H, 2, 257, 9, LIN + ' ' + SPLIT + ' head_fwd cq_col qkv_bwd', True, heads=H),
        row('H%d-T128-extreme' % H, 3, 128, 9, LIN + ' ' + SPLIT + ' head_fwd', True, heads=H, ragged=True)]
] + [
    # ---- the rnn head: one launch up to B = 80, chunked LSTMs for 81..256, 4-sample groups beyond (T 16 < 32: the loss seeds are launched)
    row('rnn-B80-last-one-launch', 80, 16, 6, BLK + ' ' + QL + ' head_fwd rnn_fwd rnn_bwd', False, predictor='rnn'),
    row('rnn-B81-first-chunked-lstm', 81, 16, 6, BLK + ' ' + QL + ' head_fwd lstm_fwd lstm_bwd', False, predictor='rnn'),
    row('rnn-B256-last-one-sample-lstm', 256, 16, 6, BLK + ' ' + QL + ' head_fwd lstm_fwd lstm_bwd', False, predictor='rnn'),
    row('rnn-B257-first-4-sample-groups', 257, 16, 6, BLK + ' ' + QL + ' head_fwd lstm_fwd lstm_bwd', False, predictor='rnn'),
    row('rnn-B3-T129-element-hash', 3, 129, 9, SPLIT + ' ' + QL + ' head_fwd cq_col qkv_bwd rnn_fwd rnn_bwd', True, predictor='rnn'),
    # ---- the eager loss (vsl_loss ahead of the backward, seeds read from memory)
    row('eager-T129', 3, 129, 9, SPLIT + ' head_fwd cq_col qkv_bwd ' + QL, False, lazy=False),
    row('eager-Lq33', 3, 40, 33, BLK + ' qkv_bwd cq_col ' + LIN, False, lazy=False),
]


def test_every_row_states_what_the_dispatch_predicates_select():
    for p in ROWS:
        r = p.values[0]
        assert len(set(r['want'])) == len(r['want']) and set(r['want']) <= set(ROUTE_LABELS), p.id
        assert not r['ragged'] or r['B'] >= 2, p.id
        got, inline = predicted_routes(r['B'], r['T'], r['Lq'], r['heads'], r['predictor'], r['lazy'])
        assert set(r['want']) == got and r['inline'] == inline, (p.id, sorted(got), inline)


def _check(r, param_seed, batch_seed, step_seed, scaled_bias_floor, context, **cfg):
    check_training_against_oracle(r['B'], r['T'], r['Lq'], r.get('Lc', 6),
                                  cfg=dict(num_heads=r['heads'], predictor=r['predictor'], video_feature_dim=r['Dv'], word_dim=r['word_dim'], **cfg),
                                  param_seed=param_seed, batch_seed=batch_seed, step_seed=step_seed, lazy=r['lazy'],
                                  transform=extreme_ragged if r['ragged'] else None, scaled_bias_floor=scaled_bias_floor,
                                  want=r['want'], never=tuple(n for n in ROUTE_LABELS if n not in r['want']), seeds_inline=r['inline'],
                                  context=context)


@pytest.mark.gpu
@pytest.mark.parametrize('r', ROWS)
def test_training_step_at_a_dispatch_boundary(r, request):
    _check(r, 101, 102, (3 << 33) + 777, False, request.node.callspec.id)


# ---- the training-mode random sweep (tests/test_fuzz_parity.py draws the eval-mode one)
SWEEP_SEED, SWEEP_N = 2027, 20


def sweep_shapes(n=SWEEP_N, seed=SWEEP_SEED):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        T = int(rs.choice([4, 16, 31, 32, 33, 64, 97, 128, 129, 250, 255, 256, 257, 300, 384, 520]))
        s = dict(heads=int(rs.choice([4, 8, 8, 16])), B=int(rs.randint(1, 5)) if T <= 256 else int(rs.randint(1, 3)), T=T,
                 Lq=int(rs.choice([1, 2, 9, 20, 31, 32, 33, 47, 64, 65, 96, 97, 128])), Lc=int(rs.choice([4, 5, 10, 17, 24, 25, 40])),
                 Dv=int(rs.choice([4, 36, 64, 100, 500, 1024])), char_dim=int(rs.choice([50, 50, 8, 64, 65, 100, 128])),
                 char_size=int(rs.choice([40, 40, 17, 97, 200])), word_table=bool(rs.randint(0, 3) == 0),
                 ragged=i % 3 == 2, lazy=(i + i // 4) % 2 == 0, predictor='rnn' if i % 4 == 3 else 'transformer', word_dim=300)
        if s['ragged']:
            s['B'] = max(s['B'], 2)
        want, s['inline'] = predicted_routes(s['B'], s['T'], s['Lq'], s['heads'], s['predictor'], s['lazy'])
        s['want'] = tuple(sorted(want))
        s['name'] = 'sweep%d-H%d-B%d-T%d-Lq%d%s%s%s' % (i, s['heads'], s['B'], T, s['Lq'], '-rnn' if s['predictor'] == 'rnn' else '',
                                                       '-extreme' if s['ragged'] else '', '-lazy' if s['lazy'] else '-eager')
        out.append(s)
    return out


def test_the_sweep_reaches_every_route():
    seen = set()
    for s in sweep_shapes():
        seen |= set(s['want'])
    assert seen == set(ROUTE_LABELS) - {'lstm_fwd', 'lstm_bwd'}, sorted(set(ROUTE_LABELS) - seen)     # (B > 80 is the table's business)


@pytest.mark.gpu
@pytest.mark.parametrize('s', sweep_shapes(), ids=lambda s: s['name'])
def test_training_mode_random_shape(s):
    # scaled_bias_floor: tiny shapes with cancelling Conv1D bias sums are judged by their summands (tests/test_fuzz_parity.py)
    _check(s, 201, 202, (9 << 33) + 4242, True, s['name'], char_dim=s['char_dim'], char_size=s['char_size'], word_table=s['word_table'])
