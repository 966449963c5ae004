"""Evaluation-forward rate: `model.eval()` + `torch.no_grad()` + `extract_index` (what runner.eval_test runs per batch), the inference mode of
this build against a baseline library without it, on the same box in the same call.

    python tools/build_base.py <parent revision>            # -> vslnet_amd/lib/libvslnet_hip_base.so (has no vsl_inference_workspace_floats)
    python tools/infer_rate.py [--base vslnet_amd/lib/libvslnet_hip_base.so] [--out profiles/infer_rate.txt] [--commit <hash>]

Per shape: base / new / base / new, every measurement a fresh child process under its own time limit, one after the other; the script stops at
the first child that does not exit with 0.  A child keeps `--resident` distinct synthetic batches in HBM and rotates them (as bench.py does),
warms up, sizes a region to at least 0.5 s, times five device-synchronised regions and reports their median.  With the baseline library loaded
through VSLNET_HIP_LIB the module's no_grad path falls back to the saved-path evaluation forward: that is the baseline.  The spread of a shape
is the difference between its two base runs; the line ends in `ok` when the new mean is not slower than the base mean by more than that.
B = 64 at T = 4096 does not fit the baseline's plan: its rate is reported against the B = 16 baseline runs of the same T."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name, predictor, B, T, Dv, resident batches, baseline shape (None: the shape itself)
SHAPES = [
    ('configs[1] B 64 T 128 Dv 1024', 'transformer', 64, 128, 1024, 10, None),
    ('configs[2] B 32 T 256 Dv 4096', 'transformer', 32, 256, 4096, 6, None),
    ('configs[4] model B 64 T 1024', 'transformer', 64, 1024, 1024, 4, None),
    ('configs[0] rnn B 16 T 128', 'rnn', 16, 128, 1024, 10, None),
    ('long video B 16 T 4096', 'transformer', 16, 4096, 1024, 3, None),
    ('long video B 64 T 4096', 'transformer', 64, 4096, 1024, 2, 'long video B 16 T 4096'),
]
LQ, LC = 20, 10


def child(predictor, B, T, Dv, nres, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.synthetic import make_configs, synthetic_batch
    configs = make_configs(video_feature_dim=Dv, max_pos_len=max(T, LQ), predictor=predictor)
    torch.manual_seed(configs.seed)
    glove = torch.randn(configs.word_size - 2, configs.word_dim).numpy()
    model = VSLNet(configs, glove).cuda().eval()
    batches = [synthetic_batch(configs, B, T, LQ, LC, seed=100 + 1000 * k) for k in range(nres)]

    def run(n, first=0):
        with torch.no_grad():
            for i in range(first, first + n):
                b = batches[i % nres]
                _, sl, el = model(b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'])
                model.extract_index(sl, el)
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
    eng = model._engine
    mode = 'inference' if eng.has_inference and eng.use_inference else 'saved path'
    assert (eng.inference_forwards > 0) == (mode == 'inference')
    ws = eng.inference_workspace_floats(B, T, LQ, LC) if mode == 'inference' else eng.workspace_floats(B, T, LQ, LC)
    # one profiled forward: where the time goes
    eng.profile_select('*')
    run(3)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_select(None)
    print(json.dumps({'ms': statistics.median(times), 'regions_ms': times, 'steps': steps, 'mode': mode, 'workspace_floats': ws,
                      'device': torch.cuda.get_device_name(), 'per_launch_us': {k: 1e3 * v[0] / v[1] for k, v in prof.items()},
                      'launches': {k: v[1] // 3 for k, v in prof.items()}}))


def run_child(shape, lib, a):
    name, predictor, B, T, Dv, nres, _ = shape
    env = dict(os.environ)
    env.pop('VSLNET_HIP_LIB', None)
    if lib:
        env['VSLNET_HIP_LIB'] = lib
    cmd = [sys.executable, os.path.abspath(__file__), '--child', predictor, str(B), str(T), str(Dv), str(nres), '--min-region', str(a.min_region),
           '--regions', str(a.regions)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        return None, '%s: child timed out after %d s' % (name, a.child_timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    if r.returncode != 0 or not lines:
        return None, '%s: child exit status %d: %s' % (name, r.returncode, (r.stderr.strip().splitlines() or [''])[-1])
    return json.loads(lines[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', nargs=5)
    ap.add_argument('--min-region', type=float, default=0.5)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--base', default=os.path.join(ROOT, 'vslnet_amd', 'lib', 'libvslnet_hip_base.so'))
    ap.add_argument('--commit', default=None, help='what the record calls this build (default: git rev-parse of the checkout)')
    ap.add_argument('--only', default=None, help='comma-separated indices into SHAPES')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), int(a.child[2]), int(a.child[3]), int(a.child[4]), a.min_region, a.regions)
        return 0
    if not os.path.exists(a.base):
        print('no baseline library at %s: python tools/build_base.py <parent revision>' % a.base)
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
    emit('# evaluation forward (model.eval(), no_grad, extract_index included), Lq %d Lc %d, median of %d regions of >= %.1f s, HBM-resident batches rotated'
         % (LQ, LC, a.regions, a.min_region))
    emit('# new = %s (inference mode) ; base = %s (saved-path evaluation forward) ; base / new / base / new, one fresh process each' % (commit, os.path.basename(a.base)))
    shapes = SHAPES if a.only is None else [SHAPES[int(i)] for i in a.only.split(',')]
    base_of, rc = {}, 0
    for shape in shapes:
        name, predictor, B, T, Dv, nres, ref = shape
        res = {'base': [], 'new': []}
        err = None
        for which in (('new', 'new') if ref else ('base', 'new', 'base', 'new')):
            out, err = run_child(shape, a.base if which == 'base' else None, a)
            if err:
                break
            if not lines[0].startswith('# box'):
                lines.insert(0, '# box: ' + out['device'])
            assert out['mode'] == ('saved path' if which == 'base' else 'inference'), (which, out['mode'])
            res[which].append(out)
        if err:
            emit('STOPPED: ' + err)
            rc = 1
            break
        new = statistics.mean(o['ms'] for o in res['new'])
        if ref is None:
            b = [o['ms'] for o in res['base']]
            base, spread = statistics.mean(b), abs(b[0] - b[1])
            base_of[name] = (base, B)
            ok = new <= base + spread
            emit('%-32s base %8.3f %8.3f ms  new %8.3f %8.3f ms  spread %6.3f ms  new/base %.3f  %8.1f -> %8.1f pairs/s  workspace %.3f -> %.3f GiB  %s'
                 % (name, b[0], b[1], res['new'][0]['ms'], res['new'][1]['ms'], spread, new / base, B / base * 1e3, B / new * 1e3,
                    res['base'][0]['workspace_floats'] * 4 / 2 ** 30, res['new'][0]['workspace_floats'] * 4 / 2 ** 30, 'ok' if ok else 'SLOWER'))
            rc = rc or (0 if ok else 3)
        else:
            base, bB = base_of.get(ref, (None, None))
            emit('%-32s new %8.3f %8.3f ms  %8.1f pairs/s  workspace %.3f GiB  (no baseline: the training plan refuses B %d)%s'
                 % (name, res['new'][0]['ms'], res['new'][1]['ms'], B / new * 1e3, res['new'][0]['workspace_floats'] * 4 / 2 ** 30, B,
                    '' if base is None else '  against %d base calls at B %d: %.3f ms, %.1f pairs/s -> x %.3f' % (B // bB, bB, base * (B // bB), bB / base * 1e3,
                                                                                                              base * (B // bB) / new)))
        for which in ('base', 'new'):
            if res[which]:
                o = res[which][0]
                top = sorted(o['per_launch_us'].items(), key=lambda kv: -kv[1] * o['launches'][kv[0]])[:8]
                emit('    %-4s per launch: ' % which + '  '.join('%s %.1f us x %d' % (k, v, o['launches'][k]) for k, v in top))
        flush()
    flush()
    return rc


if __name__ == '__main__':
    sys.exit(main())
