"""Coarse-to-fine corpus search: `retrieve(prefilter=M)` on this build (B) against the exhaustive `retrieve` on the PARENT library (A), the first stage's
cost per pair, and `select_topm` against `torch.topk`.

    python tools/build_base.py <parent>                                   # A runs the PARENT library: lib/libvslnet_hip_base.so
    python tools/prefilter_rate.py [--out profiles/prefilter_rate.txt] [--only retrieve,highlight,select] [--base PATH] [--commit <hash>]

The protocol of tools/retrieve_rate.py: every measurement a fresh child process under its own time limit, one after the other; the script stops at the
first child that does not exit with 0.  A child warms up, sizes a region to at least 0.5 s, times five device-synchronised regions and reports their
median.  The spread of a row is the difference between its two A runs; a B within it is "level".

retrieve: configs[1]'s model, T = 128, Q = 64 queries, k = 5, chunks of 4096 pairs, N in {64, 1024} synthetic videos (encoded once, resident), M in
{8, 64}.  Per N: A / B(M = 8) / B(M = 64), twice.  A = `retrieve(prefilter=0)` through the parent library (that path needs no new symbol), B =
`retrieve(prefilter=M)`; both include the copy of the (Q, k) result.  The query encodings are resident in both: the search alone is timed.
highlight: 64 queries x 64 videos = 4096 pairs in ONE call: A = the parent's `localize_pairs`, B = `highlight_pairs` (the first stage), per pair.
select: `select_topm` of a (64, N) matrix, M = 64, against `torch.topk(64, sorted=True)` on the same tensor.  torch.topk has no tie rule: equal keys come
back in an unspecified order, so the two do different work on ties (the keys here are random and distinct)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from localize_rate import LC, LQ, _model, _timed      # noqa: E402  (the same model and timing loop)

SHAPE = dict(Q=64, T=128, Dv=1024, k=5, pairs_per_call=4096)
CORPORA = (64, 1024)
KEEP = (8, 64)
SELECT = ((64, 1024), (64, 65536))


def _corpus(N):
    """configs[1]'s model, N resident video encodings (encoded 64 at a time) and 64 resident query encodings"""
    import torch
    from vslnet_amd.engine import VideoEncoding
    from vslnet_amd.synthetic import synthetic_batch
    S = SHAPE
    configs, model = _model('transformer', S['T'], S['Dv'])
    with torch.no_grad():
        enc, mask = [], []
        for c in range(0, N, 64):
            b = synthetic_batch(configs, 64, S['T'], LQ, LC, seed=77 + c)
            e = model.encode_video(b['vfeats'][:min(64, N - c)].contiguous(), b['v_mask'][:min(64, N - c)].contiguous())
            enc.append(e.encoding)
            mask.append(e.v_mask)
        venc = VideoEncoding(torch.cat(enc).contiguous(), torch.cat(mask).contiguous(), owner=model, epoch=model._param_epoch)
        b = synthetic_batch(configs, S['Q'], S['T'], LQ, LC, seed=78)
        qenc = model.encode_query(b['word_ids'], b['char_ids'], b['q_mask'])
    return model, venc, qenc


def child_retrieve(N, M, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model, venc, qenc = _corpus(N)
    S = SHAPE

    def run(m, first=0):
        with torch.no_grad():
            for _ in range(m):
                model.retrieve(venc, qenc, S['k'], nms_iou=0.5, pairs_per_call=S['pairs_per_call'], **({'prefilter': M} if M else {})).tag.cpu()
    ms, times, steps = _timed(run, min_region_s, regions)
    print(json.dumps({'ms': ms, 'regions_ms': times, 'steps': steps, 'device': torch.cuda.get_device_name()}))


def child_highlight(what, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model, venc, qenc = _corpus(64)
    Q = SHAPE['Q']
    qidx = torch.arange(Q, dtype=torch.int32, device='cuda').repeat_interleave(64)
    vidx = torch.arange(64, dtype=torch.int32, device='cuda').repeat(Q)
    eng = model._engine_for(venc.encoding.device)
    matrix = torch.empty(Q, 64, device='cuda')

    def run(m, first=0):
        with torch.no_grad():
            for _ in range(m):
                if what == 'A':
                    model.localize_pairs(venc, qenc, vidx, qidx)
                else:
                    eng.highlight_pairs(model._flat, venc, qenc, vidx, qidx, out=matrix, ld=64)
    ms, times, steps = _timed(run, min_region_s, regions)
    eng.profile_select('*')
    run(3)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_select(None)
    print(json.dumps({'ms': ms, 'regions_ms': times, 'steps': steps, 'device': torch.cuda.get_device_name(),
                      'per_launch_us': {k: 1e3 * v[0] / v[1] for k, v in prof.items()}, 'launches': {k: v[1] // 3 for k, v in prof.items()}}))


def child_select(what, G, N, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    from vslnet_amd.engine import Engine
    from vslnet_amd.synthetic import make_configs
    eng = Engine(make_configs(video_feature_dim=64))
    key = torch.rand(G, N, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3))

    def run(m, first=0):
        for _ in range(m):
            if what == 'torch':
                key.topk(64, dim=1, sorted=True)
            else:
                eng.select_topm(key, 64)
    ms, times, steps = _timed(run, min_region_s, regions)
    print(json.dumps({'ms': ms, 'regions_ms': times, 'steps': steps, 'device': torch.cuda.get_device_name()}))


def run_child(args, a, name, env_extra=None):
    env = dict(os.environ)
    env.pop('VSLNET_HIP_LIB', None)
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.abspath(__file__), '--child'] + [str(x) for x in args] + ['--min-region', str(a.min_region), '--regions', str(a.regions)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        return None, '%s: child timed out after %d s' % (name, a.child_timeout)
    lines = [x for x in r.stdout.splitlines() if x.startswith('{')]
    if r.returncode != 0 or not lines:
        return None, '%s: child exit status %d: %s' % (name, r.returncode, (r.stderr.strip().splitlines() or [''])[-1])
    return json.loads(lines[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', nargs='+')
    ap.add_argument('--min-region', type=float, default=0.5)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--base', default=os.path.join(ROOT, 'vslnet_amd', 'lib', 'libvslnet_hip_base.so'), help='the parent library (tools/build_base.py <parent>)')
    ap.add_argument('--commit', default=None)
    ap.add_argument('--only', default=None, help='comma-separated: retrieve, highlight, select')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        kind = a.child[0]
        if kind == 'retrieve':
            child_retrieve(int(a.child[1]), int(a.child[2]), a.min_region, a.regions)
        elif kind == 'highlight':
            child_highlight(a.child[1], a.min_region, a.regions)
        else:
            child_select(a.child[1], int(a.child[2]), int(a.child[3]), a.min_region, a.regions)
        return 0
    if not os.path.exists(a.base):
        print('no parent library at %s: python tools/build_base.py <parent> first' % a.base)
        return 2
    base = {'VSLNET_HIP_LIB': a.base}
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

    def series(jobs, name):
        """jobs: (label, child args, env) run in order, twice -> {label: [out, out]}, or None after a failed child"""
        res = {label: [] for label, _, _ in jobs}
        for _ in range(2):
            for label, args, env in jobs:
                out, err = run_child(args, a, '%s %s' % (name, label), env)
                if err:
                    emit('STOPPED: ' + err)
                    return None
                if not lines[0].startswith('# box'):
                    lines.insert(0, '# box: ' + out['device'])
                res[label].append(out)
        return res
    S = SHAPE
    emit('# %s on top of its parent.  Evaluation calls (model.eval(), no_grad), Lq %d Lc %d, median of %d regions of >= %.1f s, every measurement one fresh process,'
         % (commit, LQ, LC, a.regions, a.min_region))
    emit('# the runs of a row interleaved (A / B.. / A / B..).  spread(A) = the difference of the two A runs: a B within it of A is level')
    only = None if a.only is None else a.only.split(',')
    if only is None or 'retrieve' in only:
        emit('# retrieve: %d queries, T %d, Dv %d, k %d, chunks of %d pairs, encodings resident.  A = retrieve(prefilter=0) on the PARENT library ; B = retrieve(prefilter=M)'
             % (S['Q'], S['T'], S['Dv'], S['k'], S['pairs_per_call']))
        for N in CORPORA:
            res = series([('A', ['retrieve', N, 0], base)] + [('M%d' % M, ['retrieve', N, M], None) for M in KEEP], 'retrieve N %d' % N)
            if res is None:
                return 1
            am = [o['ms'] for o in res['A']]
            A, spread = statistics.mean(am), abs(am[0] - am[1])
            for M in KEEP:
                bm = [o['ms'] for o in res['M%d' % M]]
                Bm = statistics.mean(bm)
                emit('retrieve N %4d  M %2d   A %9.3f %9.3f ms  B %9.3f %9.3f ms  spread(A) %7.3f ms  B/A %.3f  %s'
                     % (N, M, am[0], am[1], bm[0], bm[1], spread, Bm / A, 'faster' if Bm < A - spread else 'level' if Bm <= A + spread else 'SLOWER'))
    if only is None or 'highlight' in only:
        res = series([('A', ['highlight', 'A'], base), ('B', ['highlight', 'B'], None)], 'highlight')
        if res is None:
            return 1
        am, bm = [o['ms'] for o in res['A']], [o['ms'] for o in res['B']]
        emit('# first stage, 4096 pairs (64 queries x 64 videos) in one call: A = localize_pairs on the PARENT library, B = highlight_pairs into the (Q, N) matrix')
        emit('highlight_pairs 4096 pairs    A %8.3f %8.3f ms  B %8.3f %8.3f ms  spread(A) %6.3f ms  B/A %.3f   per pair: A %.3f us  B %.3f us'
             % (am[0], am[1], bm[0], bm[1], abs(am[0] - am[1]), statistics.mean(bm) / statistics.mean(am), 1e3 * statistics.mean(am) / 4096, 1e3 * statistics.mean(bm) / 4096))
        for which in ('A', 'B'):
            o = res[which][0]
            top = sorted(o['per_launch_us'].items(), key=lambda kv: -kv[1] * o['launches'][kv[0]])[:9]
            emit('    %s per launch: ' % which + '  '.join('%s %.1f us x %d' % (k, v, o['launches'][k]) for k, v in top))
    if only is None or 'select' in only:
        emit('# select_topm (G, N) M 64 against torch.topk(64, sorted=True): ms per call, back to back on one stream.  torch.topk has no tie rule (random distinct keys here)')
        for G, N in SELECT:
            res = series([('torch', ['select', 'torch', G, N], None), ('kernel', ['select', 'kernel', G, N], None)], 'select (%d, %d)' % (G, N))
            if res is None:
                return 1
            am, bm = [o['ms'] for o in res['torch']], [o['ms'] for o in res['kernel']]
            emit('select_topm G %3d N %6d M 64   torch.topk %8.4f %8.4f ms   kernel %8.4f %8.4f ms   kernel / torch %.3f'
                 % (G, N, am[0], am[1], bm[0], bm[1], statistics.mean(bm) / statistics.mean(am)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
