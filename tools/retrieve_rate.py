"""Searching a corpus: `localize_pairs` on resident query AND video encodings (B) against `localize` on a replicated query batch (A), the cost of
`encode_query`, `merge_topk` against a torch composition, and one whole `retrieve`.

    python tools/build_base.py <parent>                                   # A runs the PARENT library: lib/libvslnet_hip_base.so
    python tools/retrieve_rate.py [--out profiles/retrieve_rate.txt] [--only 0,1,merge,retrieve] [--base PATH] [--commit <hash>]

The protocol of tools/localize_rate.py: per item A / B / A / B, every measurement a fresh child process under its own time limit, one after the other;
the script stops at the first child that does not exit with 0.  A child keeps `resident` distinct batches in HBM and rotates them, warms up, sizes a
region to at least 0.5 s, times five device-synchronised regions and reports their median.  The spread of a row is the difference between its two A runs.

Per-call time.  B pairs = B / 4 queries, each asked about 4 of B / 4 videos.  A = the parent library's `localize` on the replicated batch
word_ids[query_index] against the resident video encoding; B = this build's `localize_pairs` on the resident encodings of both sides; both include
`extract_index`, the indices are device tensors.  `encode_query` is timed on B queries per call and reported per query; break-even = encode ms per
query / ((A - B) / B): how many videos a query must be asked about before encoding it once is paid back.  A row ends in `ok` when B is no slower
than A by more than the spread.

merge_topk: B lists of K slots into G groups of K_out, against the torch composition on the same device tensors -- mask by count, `topk` over the
flattened group, gather (it does not implement the tag / list tie rule and needs the lists grouped contiguously).  Reported, no ratio promised;
`cached` / `rescan` = the kernel with and without its per-thread cached heads (VSL_MERGE_RESCAN_ALL=1).

retrieve: 64 queries x 64 videos at T = 128, k 5: A = the same chunks through the parent's `localize` on replicated queries + `extract_topk` + a
host merge (one (pairs, k) device-to-host copy and a Python sort per query); B = VSLNet.retrieve."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from localize_rate import LC, LQ, SHAPES, _model, _timed      # noqa: E402  (the same shapes, model and timing loop)

MERGE_SHAPES = [(4096, 5, 64, 10), (64, 5, 1, 5)]
RETRIEVE = dict(Q=64, N=64, T=128, Dv=1024, k=5, pairs_per_call=1024)


def child_pairs(what, predictor, B, T, Dv, nres, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from vslnet_amd.synthetic import synthetic_batch
    configs, model = _model(predictor, T, Dv)
    n = max(1, B // 4)
    batches = [synthetic_batch(configs, B, T, LQ, LC, seed=100 + 1000 * k) for k in range(nres)]
    qidx = (torch.arange(B, device='cuda') // 4 % n).to(torch.int32)
    vidx = (torch.arange(B, device='cuda') % n).to(torch.int32)
    with torch.no_grad():
        if what != 'EQ':
            vencs = [model.encode_video(b['vfeats'][:n].contiguous(), b['v_mask'][:n].contiguous()) for b in batches]
        for b in batches:
            del b['vfeats']
        if what == 'A':
            rep = [tuple(b[k][:n][qidx.long()].contiguous() for k in ('word_ids', 'char_ids', 'q_mask')) for b in batches]

            def run(m, first=0):
                with torch.no_grad():
                    for i in range(first, first + m):
                        _, sl, el = model.localize(vencs[i % nres], vidx, *rep[i % nres])
                        model.extract_index(sl, el)
        elif what == 'B':
            qencs = [model.encode_query(b['word_ids'][:n].contiguous(), b['char_ids'][:n].contiguous(), b['q_mask'][:n].contiguous()) for b in batches]

            def run(m, first=0):
                with torch.no_grad():
                    for i in range(first, first + m):
                        _, sl, el = model.localize_pairs(vencs[i % nres], qencs[i % nres], vidx, qidx)
                        model.extract_index(sl, el)
        else:
            def run(m, first=0):
                with torch.no_grad():
                    for i in range(first, first + m):
                        b = batches[i % nres]
                        model.encode_query(b['word_ids'], b['char_ids'], b['q_mask'])
    ms, times, steps = _timed(run, min_region_s, regions)
    eng = model._engine
    eng.profile_select('*')
    run(3)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_select(None)
    ws = {'A': lambda: eng.localize_workspace_floats(B, T, LQ, LC), 'B': lambda: eng.pairs_workspace_floats(B, T, LQ),
          'EQ': lambda: eng.encode_query_workspace_floats(B, LQ, LC)}[what]()
    print(json.dumps({'ms': ms, 'regions_ms': times, 'steps': steps, 'workspace_floats': ws, 'device': torch.cuda.get_device_name(),
                      'per_launch_us': {k: 1e3 * v[0] / v[1] for k, v in prof.items()}, 'launches': {k: v[1] // 3 for k, v in prof.items()}}))


def child_merge(what, B, K, G, K_out, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    from vslnet_amd.engine import Engine, TopkSpans
    from vslnet_amd.synthetic import make_configs
    eng = Engine(make_configs(video_feature_dim=64))
    gen = torch.Generator(device='cuda').manual_seed(3)
    per = B // G                                                   # lists of a group are contiguous (the torch composition needs that)
    prob = torch.rand(B, K, device='cuda', generator=gen).sort(dim=1, descending=True).values
    count = torch.randint(1, K + 1, (B,), device='cuda', generator=gen, dtype=torch.int32)
    start = torch.randint(0, 100, (B, K), device='cuda', generator=gen)
    spans = TopkSpans(start, start + 5, prob.log(), prob, count)
    group = (torch.arange(B, device='cuda') // per).to(torch.int32)
    tag = torch.arange(B, device='cuda', dtype=torch.int32)
    if what == 'torch':
        def run(m, first=0):
            for _ in range(m):
                key = torch.where(torch.arange(K, device='cuda')[None, :] < count[:, None], prob, torch.full_like(prob, -1.0)).view(G, per * K)
                val, pos = key.topk(K_out, dim=1)
                torch.gather(spans.start.view(G, per * K), 1, pos), torch.gather(spans.end.view(G, per * K), 1, pos)
                torch.gather(spans.score.view(G, per * K), 1, pos), pos // K, (val >= 0).sum(dim=1)
    else:
        def run(m, first=0):
            for _ in range(m):
                eng.merge_topk(spans, group, G, K_out, tag=tag)
    ms, times, steps = _timed(run, min_region_s, regions)
    print(json.dumps({'ms': ms, 'regions_ms': times, 'steps': steps, 'device': torch.cuda.get_device_name()}))


def child_retrieve(what, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from vslnet_amd.synthetic import synthetic_batch
    R = RETRIEVE
    Q, N, k = R['Q'], R['N'], R['k']
    configs, model = _model('transformer', R['T'], R['Dv'])
    b = synthetic_batch(configs, max(Q, N), R['T'], LQ, LC, seed=77)
    with torch.no_grad():
        venc = model.encode_video(b['vfeats'][:N].contiguous(), b['v_mask'][:N].contiguous())
        lengths = venc.v_mask.sum(dim=1).to(torch.int32)
        q = tuple(b[x][:Q].contiguous() for x in ('word_ids', 'char_ids', 'q_mask'))
        if what == 'B':
            def run(m, first=0):
                with torch.no_grad():
                    for _ in range(m):
                        qenc = model.encode_query(*q)              # (the query encodings are part of the search)
                        model.retrieve(venc, qenc, k, nms_iou=0.5, pairs_per_call=R['pairs_per_call']).tag.cpu()
        else:
            per = R['pairs_per_call'] // Q
            queries = torch.arange(Q, device='cuda')

            def run(m, first=0):
                with torch.no_grad():
                    for _ in range(m):
                        rows = []
                        for v0 in range(0, N, per):
                            nv = min(per, N - v0)
                            qidx = queries.repeat_interleave(nv)
                            vidx = torch.arange(v0, v0 + nv, device='cuda').repeat(Q)
                            _, sl, el = model.localize(venc, vidx.to(torch.int32), *(t[qidx] for t in q))
                            s = model.extract_topk(sl, el, k, nms_iou=0.5, lengths=lengths[vidx], want_prob=True)
                            rows.append(torch.cat([qidx[:, None].double().expand(-1, k), vidx[:, None].double().expand(-1, k), s.start.double(), s.end.double(),
                                                   s.prob.double()], dim=1).cpu().numpy())
                        allr = np.concatenate(rows).reshape(-1, 5, k)
                        for qq in range(Q):                        # the host merge: one sort per query
                            mine = allr[allr[:, 0, 0] == qq]
                            sorted(zip(-mine[:, 4].reshape(-1), mine[:, 1].reshape(-1), mine[:, 2].reshape(-1), mine[:, 3].reshape(-1)))[:k]
    ms, times, steps = _timed(run, min_region_s, regions)
    print(json.dumps({'ms': ms, 'regions_ms': times, 'steps': steps, 'device': torch.cuda.get_device_name()}))


def run_child(args, a, name, env_extra=None):
    env = dict(os.environ)
    env.pop('VSLNET_HIP_LIB', None)
    env.pop('VSL_MERGE_RESCAN_ALL', None)
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
    ap.add_argument('--only', default=None, help='comma-separated indices into SHAPES, `merge`, `retrieve`')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        kind = a.child[0]
        if kind == 'pairs':
            what, predictor, B, T, Dv, nres = a.child[1:]
            child_pairs(what, predictor, int(B), int(T), int(Dv), int(nres), a.min_region, a.regions)
        elif kind == 'merge':
            child_merge(a.child[1], *(int(x) for x in a.child[2:]), a.min_region, a.regions)
        else:
            child_retrieve(a.child[1], a.min_region, a.regions)
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

    def four(argsA, argsB, name, envA=None, envB=None):
        res = {'A': [], 'B': []}
        for which in ('A', 'B', 'A', 'B'):
            out, err = run_child(argsA if which == 'A' else argsB, a, name + ' ' + which, envA if which == 'A' else envB)
            if err:
                emit('STOPPED: ' + err)
                return None
            if not lines[0].startswith('# box'):
                lines.insert(0, '# box: ' + out['device'])
            res[which].append(out)
        return res
    emit('# %s on top of its parent.  Evaluation calls (model.eval(), no_grad), Lq %d Lc %d, median of %d regions of >= %.1f s, HBM-resident batches rotated, A / B / A / B,'
         % (commit, LQ, LC, a.regions, a.min_region))
    emit('# one fresh process each.  A = the PARENT library: localize on the replicated queries ; B = localize_pairs on resident encodings of both sides ; B pairs =')
    emit('# B / 4 queries x 4 of B / 4 videos ; extract_index included.  encode = encode_query on B queries per call, per query.  break-even = encode / ((A - B) / B)')
    only = None if a.only is None else a.only.split(',')
    rc = 0
    for i, (name, predictor, B, T, Dv, nres) in enumerate(SHAPES):
        if only is not None and str(i) not in only:
            continue
        enc, err = run_child(['pairs', 'EQ', predictor, B, T, Dv, nres], a, name + ' encode_query')
        if err:
            emit('STOPPED: ' + err)
            return 1
        per_query = enc['ms'] / B
        emit('%-30s encode_query: %8.3f ms per call of %d queries = %.4f ms per query   workspace %.3f GiB' % (name, enc['ms'], B, per_query, enc['workspace_floats'] * 4 / 2 ** 30))
        emit('    encode per launch: ' + '  '.join('%s %.1f us x %d' % (k, v, enc['launches'][k]) for k, v in sorted(enc['per_launch_us'].items(), key=lambda kv: -kv[1])[:5]))
        res = four(['pairs', 'A', predictor, B, T, Dv, nres], ['pairs', 'B', predictor, B, T, Dv, nres], name, envA=base)
        if res is None:
            return 1
        am, bm = [o['ms'] for o in res['A']], [o['ms'] for o in res['B']]
        A, Bm, spread = statistics.mean(am), statistics.mean(bm), abs(am[0] - am[1])
        ok = Bm <= A + spread
        saving = (A - Bm) / B
        emit('%-30s A %8.3f %8.3f ms  B %8.3f %8.3f ms  spread(A) %6.3f ms  B/A %.3f  saving %.4f ms per pair  break-even %s videos per query  workspace %.3f -> %.3f GiB  %s'
             % (name, am[0], am[1], bm[0], bm[1], spread, Bm / A, saving, ('%.2f' % (per_query / saving)) if saving > 0 else 'none',
                res['A'][0]['workspace_floats'] * 4 / 2 ** 30, res['B'][0]['workspace_floats'] * 4 / 2 ** 30, 'ok' if ok else 'DEFECT'))
        for which in ('A', 'B'):
            o = res[which][0]
            top = sorted(o['per_launch_us'].items(), key=lambda kv: -kv[1] * o['launches'][kv[0]])[:9]
            emit('    %s per launch: ' % which + '  '.join('%s %.1f us x %d' % (k, v, o['launches'][k]) for k, v in top))
        rc = rc or (0 if ok else 3)
    if only is None or 'merge' in only:
        emit('# merge_topk (B lists, K slots, G groups, K_out): ms per call, back to back on one stream (launch-bound: the host enqueues as fast as it can).  A = torch')
        emit('# composition (where + topk + 3 gathers + 2 small ops), B = the kernel with cached heads ; rescan = the kernel without them, one run')
        for shape in MERGE_SHAPES:
            res = four(['merge', 'torch', *shape], ['merge', 'cached', *shape], 'merge %s' % (shape,))
            if res is None:
                return 1
            resc, err = run_child(['merge', 'rescan', *shape], a, 'merge rescan', {'VSL_MERGE_RESCAN_ALL': '1'})
            if err:
                emit('STOPPED: ' + err)
                return 1
            am, bm = [o['ms'] for o in res['A']], [o['ms'] for o in res['B']]
            emit('merge_topk B %4d K %d G %2d K_out %2d   torch %8.4f %8.4f ms   kernel %8.4f %8.4f ms   kernel without cached heads %8.4f ms   kernel / torch %.3f'
                 % (*shape, am[0], am[1], bm[0], bm[1], resc['ms'], statistics.mean(bm) / statistics.mean(am)))
    if only is None or 'retrieve' in only:
        res = four(['retrieve', 'A'], ['retrieve', 'B'], 'retrieve', envA=base)
        if res is None:
            return 1
        am, bm = [o['ms'] for o in res['A']], [o['ms'] for o in res['B']]
        R = RETRIEVE
        emit('# retrieve: %d queries x %d videos at T %d, Dv %d, k %d, chunks of %d pairs.  A = the parent library: localize on replicated queries + extract_topk + one copy and a'
             % (R['Q'], R['N'], R['T'], R['Dv'], R['k'], R['pairs_per_call']))
        emit('# host sort per query ; B = encode_query + VSLNet.retrieve (+ the copy of the result).  The video encoding is resident in both')
        emit('retrieve                       A %8.3f %8.3f ms  B %8.3f %8.3f ms  spread(A) %6.3f ms  B/A %.3f' % (am[0], am[1], bm[0], bm[1], abs(am[0] - am[1]),
                                                                                                             statistics.mean(bm) / statistics.mean(am)))
    return rc


if __name__ == '__main__':
    sys.exit(main())
