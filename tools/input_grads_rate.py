"""Call time of `Engine.input_grads` (vsl_input_grads: dX = dropmask * (d_video_affine @ W), one launch of k_vproj_dx) beside what it is compared with:

    (a) the torch composition a user would write without the call, on the SAME tensors in the same process: `(G @ W) * mask`, G = the workspace's
        d_video_affine (R, 128), W = the (128, Dv) weight view of the flat bucket, mask = the (R, Dv) fp32 multiplier, materialised beforehand (its
        hashing is not charged to torch);
    (b) the training step of the shape (forward + production loss + backward), for scale.

    python tools/input_grads_rate.py [--out profiles/input_grads_rate.txt] [--commit <hash>]

Per shape two fresh child processes, A and A', one after the other, each under its own time limit; the script stops at the first child that does not
exit with 0.  A child runs one training step of a synthetic batch (drop_rate 0.2, ragged lengths), checks the call against the composition once, and
then measures every item twice in alternation: warm-up, a region sized to at least --min-region seconds, the time per call of that device-synchronised
region.  The record prints, per item, the mean of the four values and their spread (max - min over both rounds of both processes), and the kernel's own
arithmetic and store rates from the shape.  Nothing here is a gate: the record states what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# BASELINE configs[1]; configs[2]; configs[4]'s model at T 1024 (one GPU's share of its batch)
SHAPES = [('configs[1]  B 64 T 128 Dv 1024', 64, 128, 1024), ('configs[2]  B 32 T 256 Dv 4096', 32, 256, 4096), ('configs[4]  B 16 T 1024 Dv 1024', 16, 1024, 1024)]
LQ, LC = 20, 10


def child(B, T, Dv, min_region_s):
    sys.path.insert(0, ROOT)
    import torch
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.synthetic import make_configs, synthetic_batch
    configs = make_configs(video_feature_dim=Dv, max_pos_len=max(T, LQ), predictor='transformer')
    torch.manual_seed(configs.seed)
    model = VSLNet(configs, torch.randn(configs.word_size - 2, configs.word_dim).numpy()).cuda().train()
    flat, _ = model.flat_parameters
    eng = model._engine
    we = model.embedding_net.word_emb
    b = synthetic_batch(configs, B, T, LQ, LC, seed=100, ragged=True)
    msum = float(b['v_mask'].sum())
    grads = eng.new_flat()

    def step(training=True):
        eng.forward(flat, we.pad_vec.data, we.glove_vec.data, b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'], training=training, seed=777)
        _, d_h, d_sl, d_el = eng.loss(b['s_labels'], b['e_labels'], b['h_labels'], 1.0, 5.0, inv_batch=1.0 / B, mask_sum=msum, lazy=True)
        eng.backward(d_h, d_sl, d_el, grads)
    step()
    R = B * T
    out = torch.empty(B, T, Dv, device='cuda')
    eng.input_grads(out=out)
    G = eng.ws_view('d_video_affine', (R, 128))
    W = eng.views(flat)['video_affine.linear.conv1d.weight'].view(128, Dv)
    mask = (out.view(R, Dv) != 0).float() * (1.0 / (1.0 - configs.drop_rate))        # (the kernel's own zero pattern)

    def torch_dx():
        return (G @ W) * mask
    ref = torch_dx()
    dev = float((out.view(R, Dv) - ref).abs().max()) / float(ref.abs().max())
    assert dev < 1e-5, dev
    items = [('input_grads (k_vproj_dx)', lambda: eng.input_grads(out=out)), ('(a) torch (G @ W) * mask', torch_dx), ('(b) training step', step)]
    us = {name: [] for name, _ in items}
    for rnd in range(2):
        for name, fn in items:
            if name.startswith('input') or name.startswith('(a)'):
                step()                                              # (both read what a backward left)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            n = max(3, int(min_region_s / ((time.perf_counter() - t0) / 3)) + 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            us[name].append(1e6 * (time.perf_counter() - t0) / n)
    # the same two on the device's clock: events around 50 back-to-back calls (no host synchronisation inside), and the kernel's own dispatch-packet
    # time from the built-in profiler
    ev = {}
    for name, fn in items[:2]:
        step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            fn()
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ev[name] = 1e3 * e0.elapsed_time(e1) / 50
    kernel_us = []
    for training in (True, False):                  # (behind an eval-mode step the kernel hashes nothing: the multiplier is 1)
        step(training)
        eng.profile_select('vproj_dx')
        for _ in range(20):
            eng.input_grads(out=out)
        torch.cuda.synchronize()
        ms, n = eng.profile_read()['vproj_dx']
        eng.profile_select(None)
        kernel_us.append(1e3 * ms / n)
    print(json.dumps({'us': us, 'events_us': ev, 'kernel_us': kernel_us[0], 'kernel_eval_us': kernel_us[1], 'device': torch.cuda.get_device_name(), 'dropped': float((mask == 0).float().mean()), 'dev': dev}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', nargs=3)
    ap.add_argument('--min-region', type=float, default=0.3)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--commit', default=None, help='what the record calls this build (default: git rev-parse of the checkout)')
    ap.add_argument('--only', default=None, help='comma-separated indices into SHAPES')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.min_region)
        return 0
    commit = a.commit
    if commit is None:
        r = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else 'unknown'
    lines = []

    def emit(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
        if a.out:
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    emit('# input_grads call time (%s) after one training step of a synthetic batch (drop_rate 0.2, ragged lengths, Lq %d Lc %d); us per call of a' % (commit, LQ, LC))
    emit('# device-synchronised region of >= %.1f s (launch and host overhead of the call included); per item: mean of 2 rounds x 2 fresh processes (A, A\'),' % a.min_region)
    emit('# spread = max - min of those four.  (a) runs on the same G, W and a materialised mask in the same process; (b) = forward + loss + backward.')
    for name, B, T, Dv in (SHAPES if a.only is None else [SHAPES[int(i)] for i in a.only.split(',')]):
        runs = []
        for _ in range(2):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', str(B), str(T), str(Dv), '--min-region', str(a.min_region)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                emit('STOPPED: %s: child timed out after %d s' % (name, a.child_timeout))
                return 1
            js = [l for l in r.stdout.splitlines() if l.startswith('{')]
            if r.returncode != 0 or not js:
                emit('STOPPED: %s: child exit status %d: %s' % (name, r.returncode, (r.stderr.strip().splitlines() or [''])[-1]))
                return 1
            runs.append(json.loads(js[-1]))
        R = B * T
        emit('%s on %s: R %d, dX %.0f MiB, %.2f GFLOP, %.1f %% of dX exactly zero (dropped features, and padded clips the gradient does not reach); call vs composition: max |diff| / |dX|inf %.1e'
             % (name, runs[0]['device'], R, R * Dv * 4 / 2 ** 20, 2e-9 * R * 128 * Dv, 100 * runs[0]['dropped'], runs[0]['dev']))
        mean = {}
        for item in runs[0]['us']:
            v = runs[0]['us'][item] + runs[1]['us'][item]
            mean[item] = sum(v) / len(v)
            emit('    %-28s %10.1f us   spread %8.1f us   (%s)' % (item, mean[item], max(v) - min(v), ' '.join('%.1f' % x for x in v)))
        for item in runs[0]['events_us']:
            v = [r['events_us'][item] for r in runs]
            emit('    %-28s %10.1f us   between device events around 50 back-to-back calls (%s)' % (item, sum(v) / len(v), ' '.join('%.1f' % x for x in v)))
        k = [r['kernel_us'] for r in runs]
        emit('    %-28s %10.1f us   the kernel\'s own dispatch-packet time, mean of 20 launches (%s)' % ('k_vproj_dx alone', sum(k) / len(k), ' '.join('%.1f' % x for x in k)))
        mean['kernel'] = sum(k) / len(k)
        k = [r['kernel_eval_us'] for r in runs]
        emit('    %-28s %10.1f us   the same behind an eval-mode step: no dropout, the kernel hashes nothing (%s)' % ('k_vproj_dx alone, eval', sum(k) / len(k), ' '.join('%.1f' % x for x in k)))
        t = mean['input_grads (k_vproj_dx)']
        emit('    -> %.2f x the torch composition\'s time per call, %.1f %% of the step; at the kernel\'s own time %.1f TFLOP/s fp32 and %.2f TB/s of stores'
             % (t / mean['(a) torch (G @ W) * mask'], 100 * t / mean['(b) training step'], 2e-6 * R * 128 * Dv / mean['kernel'], R * Dv * 4e-6 / mean['kernel']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
