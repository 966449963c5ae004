"""Long videos: training-step rate at T = 1024, 2048 and 4096 (configs[4]'s model: Dv=1024, Lq=20, Lc=10, transformer, 8 heads, drop 0.2,
train mode), at the largest power-of-two B whose workspace fits beside the model, with vsl_workspace_floats at each shape, and the attn_bwd
ledger time (Engine.profile_select) of the query-major dQ path against the slab path (VSL_ATTN_DQ_SLABS=1) at T = 2048.

Every measurement runs in a fresh child process under its own time limit (the slab switch is read once per process):

    python tools/long_rate.py [--steps 10] [--regions 3] [--out profiles/long_rate.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [1024, 2048, 4096]
KERNELS = ('attn_fwd', 'attn_out_fwd', 'attn_bwd', 'attn_out_bwd', 'qkv_bwd', 'convblock_bwd')


def child(T, B, steps, regions):
    sys.path.insert(0, ROOT)
    import ctypes
    import torch
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.synthetic import make_configs, synthetic_batch
    configs = make_configs(video_feature_dim=1024, max_pos_len=T, drop_rate=0.2, predictor='transformer', num_heads=8)
    torch.manual_seed(0)
    glove = torch.randn(configs.word_size - 2, configs.word_dim).numpy()
    model = VSLNet(configs, glove).cuda().train()
    flat, grads = model.flat_parameters
    eng = model._engine
    n = ctypes.c_int64()
    rc = eng.lib.vsl_workspace_floats(eng.h, B, T, 20, 10, ctypes.byref(n))
    out = {'T': T, 'B': B, 'workspace_floats': n.value if rc == 0 else None}
    if rc != 0:
        out['error'] = eng.lib.vsl_last_error().decode()
        print(json.dumps(out))
        return
    b = synthetic_batch(configs, B, T, 20, 10, seed=1)
    pad_vec, glove_vec = model.embedding_net.word_emb.pad_vec.data, model.embedding_net.word_emb.glove_vec.data
    msum = float(b['v_mask'].sum())

    def step(i):
        eng.forward(flat, pad_vec, glove_vec, b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'], training=True, seed=i)
        _, d_h, d_sl, d_el = eng.loss(b['s_labels'], b['e_labels'], b['h_labels'], 1.0, 5.0, inv_batch=1.0 / B, mask_sum=msum)
        eng.backward(d_h, d_sl, d_el, grads)
    for i in range(3):
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
    for i in range(3):
        step(1000 + i)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_select(None)
    out['ms_per_step'] = statistics.median(times)
    out['pairs_per_s'] = B / (out['ms_per_step'] / 1e3)
    out['per_launch_us'] = {k: 1e3 * prof[k][0] / prof[k][1] for k in KERNELS if k in prof}
    out['launches_per_step'] = {k: prof[k][1] // 3 for k in KERNELS if k in prof}
    print(json.dumps(out))


def run(T, B, steps, regions, slabs=False, timeout=900):
    env = dict(os.environ)
    if slabs:
        env['VSL_ATTN_DQ_SLABS'] = '1'
    cmd = [sys.executable, os.path.abspath(__file__), '--child', str(T), str(B), '--steps', str(steps), '--regions', str(regions)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {'T': T, 'B': B, 'error': 'timeout'}, True
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    if r.returncode != 0 or not lines:
        fatal = r.returncode < 0 or r.returncode in (134, 139)          # a fault: start nothing more on the GPU
        return {'T': T, 'B': B, 'error': 'rc %d: %s' % (r.returncode, r.stderr.strip().splitlines()[-1:] if r.stderr else '')}, fatal
    return json.loads(lines[-1]), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', nargs=2, type=int)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--batches', default='1024:16,2048:8,4096:4', help='T:B list (B = the largest power of two that fits, found by --probe)')
    ap.add_argument('--probe', action='store_true', help='double B from the given value until a shape fails, and report the largest that ran')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.steps, a.regions)
        return
    lines = []

    def emit(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
    import torch
    emit('device: %s   median of %d regions x %d steps, train mode, drop 0.2, Dv=1024 Lq=20 Lc=10, transformer, 8 heads'
         % (torch.cuda.get_device_name(), a.regions, a.steps))
    del torch
    for tb in a.batches.split(','):
        T, B = (int(x) for x in tb.split(':'))
        res, fatal = run(T, B, a.steps, a.regions)
        while a.probe and not fatal and 'error' not in res:
            nxt, fatal = run(T, 2 * B, a.steps, a.regions)
            if 'error' in nxt:
                emit('T=%-5d B=%-4d does not run: %s' % (T, 2 * B, nxt['error']))
                break
            B, res = 2 * B, nxt
        if 'error' in res:
            emit('T=%-5d B=%-4d error: %s' % (T, B, res['error']))
        else:
            emit('T=%-5d B=%-4d %9.3f ms/step  %8.1f pairs/s  workspace %d floats (%.2f GiB)' % (T, B, res['ms_per_step'], res['pairs_per_s'],
                 res['workspace_floats'], res['workspace_floats'] * 4 / 2 ** 30))
            emit('    per launch: ' + '  '.join('%s %.1f us x %d' % (k, v, res['launches_per_step'][k]) for k, v in res['per_launch_us'].items()))
        if fatal:
            break
        if T == 2048 and 'error' not in res:
            sl, fatal = run(T, B, a.steps, a.regions, slabs=True)
            if 'error' in sl:
                emit('T=%-5d B=%-4d VSL_ATTN_DQ_SLABS=1 error: %s' % (T, B, sl['error']))
            else:
                emit('T=%-5d B=%-4d VSL_ATTN_DQ_SLABS=1: %9.3f ms/step  workspace %d floats (%.2f GiB)  attn_bwd %.1f us (query-major dQ: %.1f us)'
                     % (T, B, sl['ms_per_step'], sl['workspace_floats'], sl['workspace_floats'] * 4 / 2 ** 30, sl['per_launch_us']['attn_bwd'],
                        res['per_launch_us']['attn_bwd']))
            if fatal:
                break
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
