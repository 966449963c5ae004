"""Training through a shared video encoding (B) against the ordinary production step on the replicated batch (A), same box.

    python tools/build_base.py <parent> base                       # A's library: the parent commit
    python tools/shared_train_rate.py [--out profiles/shared_train_rate.txt] [--only 0,1] [--base vslnet_amd/lib/libvslnet_hip_base.so]

A is what training runs without the feature: the PARENT library (tools/build_base.py; --base names the file) on a (B, T, Dv) block in which every
video appears once per query -- forward, lazy loss, backward with the fused AdamW step (dp.backward_exchange_step), what main.train and bench.py
run.  B is this build's Engine.forward_shared over N = B / k videos, the same lazy loss and the same backward call, with k = 1, 2, 4 and 8 queries
per video; the video index is a device tensor (no upload per step).  Per shape: A / B(k = 1, 2, 4, 8) / A / B(...), every measurement a fresh child
process under its own time limit, one after the other; the script stops at the first child that does not exit with 0.  A child keeps `resident`
distinct batches in HBM and rotates them, warms up, sizes a region to at least 0.5 s, times five device-synchronised regions and reports their median.
The spread of a shape is the difference between its two A runs.  A B row ends in `faster` / `slower` only when BOTH its runs lie outside
[min(A) - spread, max(A) + spread] on the same side, otherwise in `inside the spread of A`.  Break-even = the smallest measured k whose row is
`faster` (none: no measured k is).  Also reported: the bytes of the (B, T, Dv) feature block a step no longer gathers and reads, (B - N) T Dv 4."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name, predictor, B, T, Dv, resident batches
SHAPES = [
    ('configs[1] B 64 T 128 Dv 1024', 'transformer', 64, 128, 1024, 10),
    ('configs[2] B 32 T 256 Dv 4096', 'transformer', 32, 256, 4096, 6),
    ('configs[4] model B 16 T 1024', 'transformer', 16, 1024, 1024, 4),
    ('configs[0] rnn B 16 T 128', 'rnn', 16, 128, 1024, 10),
]
QPV = (1, 2, 4, 8)
LQ, LC = 20, 10


def child(what, predictor, B, T, Dv, nres, qpv, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from vslnet_amd.dp import FlatAdamW, backward_exchange_step
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.synthetic import make_configs, synthetic_batch
    configs = make_configs(video_feature_dim=Dv, max_pos_len=max(T, LQ), drop_rate=0.2, predictor=predictor)
    torch.manual_seed(configs.seed)
    glove = torch.randn(configs.word_size - 2, configs.word_dim).numpy()
    model = VSLNet(configs, glove).cuda().train()
    flat, grads = model.flat_parameters
    eng = model._engine
    pad_vec, glove_vec = model.embedding_net.word_emb.pad_vec.data, model.embedding_net.word_emb.glove_vec.data
    N = (B + qpv - 1) // qpv
    idx = torch.arange(B, device='cuda') // qpv                       # query b asks about video b // qpv
    idx32 = idx.to(torch.int32)
    batches = [synthetic_batch(configs, B, T, LQ, LC, seed=100 + 1000 * k) for k in range(nres)]
    for b in batches:                                                  # N videos; the per-query mask and labels are those of the full-length videos
        b['video_v_mask'] = b['v_mask'][:N].contiguous()
        b['vfeats'] = b['vfeats'][:N].contiguous() if what == 'B' else b['vfeats'][:N][idx].contiguous()
        b['v_mask'] = b['video_v_mask'][idx].contiguous()
    mask_sum = float(batches[0]['v_mask'].sum().item())
    opt = FlatAdamW(flat, eng.layout, lr=configs.init_lr, num_train_steps=10 ** 7, clip_norm=configs.clip_norm, engine=eng)

    def run(n, first=0):
        for i in range(first, first + n):
            b = batches[i % nres]
            if what == 'B':
                eng.forward_shared(flat, pad_vec, glove_vec, b['word_ids'], b['char_ids'], b['vfeats'], b['video_v_mask'], b['q_mask'], idx32, training=True, seed=i)
            else:
                eng.forward(flat, pad_vec, glove_vec, b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'], training=True, seed=i)
            _, d_h, d_sl, d_el = eng.loss(b['s_labels'], b['e_labels'], b['h_labels'], 1.0, configs.highlight_lambda, inv_batch=1.0 / B, mask_sum=mask_sum, lazy=True)
            backward_exchange_step(eng, None, grads, (d_h, d_sl, d_el), opt)
    run(5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(5)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 5
    steps = max(5, int(min_region_s / per) + 1)
    times = []
    for r in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps, first=r * steps)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0) / steps)
    eng.profile_select('*')
    run(3)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_select(None)
    ws = eng.shared_workspace_floats(B, N, T, LQ, LC) if what == 'B' else eng.workspace_floats(B, T, LQ, LC)
    print(json.dumps({'ms': statistics.median(times), 'regions_ms': times, 'steps': steps, 'N': N, 'workspace_floats': ws, 'device': torch.cuda.get_device_name(),
                      'finite': bool(torch.isfinite(flat).all()), 'per_launch_us': {k: 1e3 * v[0] / v[1] for k, v in prof.items()},
                      'launches': {k: v[1] // 3 for k, v in prof.items()}}))


def run_child(args, a, name, base):
    env = dict(os.environ)
    env.pop('VSLNET_HIP_LIB', None)
    if base:
        env['VSLNET_HIP_LIB'] = os.path.abspath(a.base)
    cmd = [sys.executable, os.path.abspath(__file__), '--child'] + [str(x) for x in args] + ['--min-region', str(a.min_region), '--regions', str(a.regions)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        return None, '%s: child timed out after %d s' % (name, a.child_timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    if r.returncode != 0 or not lines:
        return None, '%s: child exit status %d: %s' % (name, r.returncode, (r.stderr.strip().splitlines() or [''])[-1])
    out = json.loads(lines[-1])
    if not out['finite']:
        return None, '%s: parameters not finite after the run' % name
    return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', nargs='+')
    ap.add_argument('--min-region', type=float, default=0.5)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--base', default=os.path.join(ROOT, 'vslnet_amd', 'lib', 'libvslnet_hip_base.so'), help="the parent commit's library (tools/build_base.py)")
    ap.add_argument('--commit', default=None, help='what the record calls this build (default: git rev-parse of the checkout)')
    ap.add_argument('--only', default=None, help='comma-separated indices into SHAPES')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        what, predictor, B, T, Dv, nres, qpv = a.child
        child(what, predictor, int(B), int(T), int(Dv), int(nres), int(qpv), a.min_region, a.regions)
        return 0
    if not os.path.exists(a.base):
        print('no parent library at %s: build it with tools/build_base.py <parent> base' % a.base, file=sys.stderr)
        return 2
    commit = a.commit
    if commit is None:
        r = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else 'unknown'
    lines = []

    def emit(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)

    def flush():
        if a.out:
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    emit('# %s.  Production training steps (forward, lazy loss, backward with the fused AdamW step; drop_rate 0.2), Lq %d Lc %d, median of %d regions of >= %.1f s,'
         % (commit, LQ, LC, a.regions, a.min_region))
    emit('# HBM-resident batches rotated.  A = the parent library, ordinary step on the replicated (B, T, Dv) block ; B = this build, forward_shared over N = B / k videos ;')
    emit('# A / B(k = %s) / A / B(...), one fresh process each.  ms are step time per batch of B queries.' % ', '.join(str(k) for k in QPV))
    only = None if a.only is None else a.only.split(',')
    for name, predictor, B, T, Dv, nres in [s for i, s in enumerate(SHAPES) if only is None or str(i) in only]:
        res = {'A': [], **{k: [] for k in QPV}}
        for rnd in range(2):
            for which in ('A',) + QPV:
                args = ['A', predictor, B, T, Dv, nres, 1] if which == 'A' else ['B', predictor, B, T, Dv, nres, which]
                out, err = run_child(args, a, '%s %s' % (name, which), base=which == 'A')
                if err:
                    emit('STOPPED: ' + err)
                    flush()
                    return 1
                if not lines[0].startswith('# box'):
                    lines.insert(0, '# box: ' + out['device'])
                res[which].append(out)
        am = [o['ms'] for o in res['A']]
        spread = abs(am[0] - am[1])
        lo, hi = min(am) - spread, max(am) + spread
        emit('%-30s A %8.3f %8.3f ms  spread(A) %6.3f ms  workspace %.3f GiB' % (name, am[0], am[1], spread, res['A'][0]['workspace_floats'] * 4 / 2 ** 30))
        breakeven = None
        for k in QPV:
            bm = [o['ms'] for o in res[k]]
            verdict = 'faster' if max(bm) < lo else 'slower' if min(bm) > hi else 'inside the spread of A'
            if verdict == 'faster' and breakeven is None:
                breakeven = k
            N = res[k][0]['N']
            emit('%-30s k %d (N %2d)  B %8.3f %8.3f ms  B/A %.3f  %s   workspace %.3f GiB  feature block not gathered %.1f MiB'
                 % (name, k, N, bm[0], bm[1], statistics.mean(bm) / statistics.mean(am), verdict, res[k][0]['workspace_floats'] * 4 / 2 ** 30, (B - N) * T * Dv * 4 / 2 ** 20))
        emit('%-30s break-even: %s' % (name, ('%d queries per video (the smallest measured k that is faster)' % breakeven) if breakeven else 'none of the measured k is faster'))
        for which in ('A', 4):
            o = res[which][0]
            top = sorted(o['per_launch_us'].items(), key=lambda kv: -kv[1] * o['launches'][kv[0]])[:10]
            emit('    %s per launch: ' % ('A' if which == 'A' else 'B k 4') + '  '.join('%s %.1f us x %d' % (kk, v, o['launches'][kk]) for kk, v in top))
        flush()
    flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
