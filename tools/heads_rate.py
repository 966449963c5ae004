"""Training-step rate at several head counts, all in one process: ms/step (median of timed regions) and the per-launch time of the attention
kernels (Engine.profile_select('*')).  Shapes: BASELINE configs[1] (B=64, T=128, Dv=1024, Lq=20, Lc=10, transformer, drop 0.2, train mode) and
configs[4] (B=16, T=1024).  At 8 heads and L <= 128 the attention core runs inside attn_block_fwd; the other head counts run attn_fwd +
attn_out_fwd.  Every ratio is against the 8-head step of the same shape, which is measured first.

    python tools/heads_rate.py [--heads 1 2 4 8 16] [--steps 20] [--regions 5]        # output committed as profiles/heads_rate.txt
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from vslnet_amd.model.VSLNet import VSLNet  # noqa: E402
from vslnet_amd.synthetic import make_configs, synthetic_batch  # noqa: E402

SHAPES = [('configs[1]', 64, 128), ('configs[4]', 16, 1024)]
KERNELS = ('attn_block_fwd', 'attn_fwd', 'attn_out_fwd', 'attn_bwd', 'attn_out_bwd', 'qkv_bwd')


def run(name, B, T, heads, steps, regions):
    configs = make_configs(video_feature_dim=1024, max_pos_len=T, drop_rate=0.2, predictor='transformer', num_heads=heads)
    torch.manual_seed(0)
    glove = torch.randn(configs.word_size - 2, configs.word_dim).numpy()
    model = VSLNet(configs, glove).cuda().train()
    flat, grads = model.flat_parameters
    eng = model._engine
    b = synthetic_batch(configs, B, T, 20, 10, seed=1)
    pad_vec, glove_vec = model.embedding_net.word_emb.pad_vec.data, model.embedding_net.word_emb.glove_vec.data
    msum = float(b['v_mask'].sum())

    def step(i):
        eng.forward(flat, pad_vec, glove_vec, b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'], training=True, seed=i)
        _, d_h, d_sl, d_el = eng.loss(b['s_labels'], b['e_labels'], b['h_labels'], 1.0, 5.0, inv_batch=1.0 / B, mask_sum=msum)
        eng.backward(d_h, d_sl, d_el, grads)
    for i in range(5):
        step(i)
    torch.cuda.synchronize()
    times = []
    for r in range(regions):
        t0 = time.perf_counter()
        for i in range(steps):
            step(100 + r * steps + i)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0) / steps)
    eng.profile_select('*')
    for i in range(5):
        step(1000 + i)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_select(None)
    per = '  '.join('%s %.1f us x %d' % (k, 1e3 * prof[k][0] / prof[k][1], prof[k][1] // 5) for k in KERNELS if k in prof)
    return statistics.median(times), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--heads', type=int, nargs='+', default=[4, 16], help='head counts to measure besides 8 (8 always runs first)')
    a = ap.parse_args()
    print('device: %s   median of %d regions x %d steps, train mode, drop 0.2' % (torch.cuda.get_device_name(), a.regions, a.steps))
    for name, B, T in SHAPES:
        ref = None
        for heads in [8] + [h for h in a.heads if h != 8]:
            ms, per = run(name, B, T, heads, a.steps, a.regions)
            ref = ms if heads == 8 else ref
            print('%-10s B=%-3d T=%-5d heads %-2d  %8.3f ms/step  (%.3fx the 8-head step)' % (name, B, T, heads, ms, ms / ref))
            print('    per launch: ' + per)
            sys.stdout.flush()


if __name__ == '__main__':
    main()
