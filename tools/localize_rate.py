"""Many queries per video: `localize` on a resident encoding (B) against the inference forward on replicated features (A), same box, same call.

    python tools/localize_rate.py [--out profiles/localize_rate.txt] [--only 0,1] [--commit <hash>]

A is what evaluation runs without the feature (`model(...)` under eval() + no_grad() on a (B, T, Dv) block in which every video appears once per
query) -- this build's inference forward, which is also the parent commit's, kernel for kernel, so no baseline library is needed.  B is
`model.localize(enc, video_index, ...)` on an (N, T, 128) encoding that `model.encode_video` left in HBM, N = ceil(B / queries per video); the video
index is a device tensor (no upload per call).  Both include `extract_index`.  Per shape and per queries-per-video (1, 4, 64): A / B / A / B, every
measurement a fresh child process under its own time limit, one after the other; the script stops at the first child that does not exit with 0.
A child keeps `resident` distinct batches (A: replicated feature blocks, B: encodings) in HBM and rotates them, warms up, sizes a region to at
least 0.5 s, times five device-synchronised regions and reports their median.  `encode_video` is timed the same way on B videos per call and
reported per video.  Break-even queries per video = encode ms per video / ((A - B) / B): how many queries a video must receive before encoding it
once is paid back.  The spread of a row is the difference between its two A runs; the row ends in `ok` when B's mean is below A's mean by more
than that (B runs a subset of A's launches plus one small gather off the dependent chain).

Last, one whole evaluation pass: runner.eval_test against runner.eval_test_shared over a resident split built here with ragged video lengths and
8 records per video.  The shared loop pads every batch to the split's longest video where eval_test pads to the batch maximum, so it processes
more rows; the figure is the net effect, reported and not gated.

`--ledger I` prints instead the critical-path ledger (tools/critical_path.py) of one inference forward and of one `localize` call of SHAPES[I]
(profiles/localize_critical_path.txt): which launches are on the dependent chain, and what the gather and the side packs cost it (nothing)."""
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
    ('configs[4] model B 64 T 1024', 'transformer', 64, 1024, 1024, 4),
    ('configs[0] rnn B 16 T 128', 'rnn', 16, 128, 1024, 10),
]
QPV = (1, 4, 64)
LQ, LC = 20, 10
EVAL = dict(n_videos=64, per_video=8, tmax=128, Dv=1024, batch=64)


def _timed(run, min_region_s, regions):
    import torch
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
    return statistics.median(times), times, steps


def _model(predictor, T, Dv):
    import torch
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.synthetic import make_configs
    configs = make_configs(video_feature_dim=Dv, max_pos_len=max(T, LQ), predictor=predictor)
    torch.manual_seed(configs.seed)
    glove = torch.randn(configs.word_size - 2, configs.word_dim).numpy()
    return configs, VSLNet(configs, glove).cuda().eval()


def child(what, predictor, B, T, Dv, nres, qpv, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from vslnet_amd.synthetic import synthetic_batch
    configs, model = _model(predictor, T, Dv)
    N = (B + qpv - 1) // qpv
    batches = [synthetic_batch(configs, B, T, LQ, LC, seed=100 + 1000 * k) for k in range(nres)]
    idx = torch.arange(B, device='cuda') // qpv                       # query b asks about video b // qpv
    with torch.no_grad():
        if what == 'A':
            # the replicated block, built once: every video once per query
            for b in batches:
                b['vfeats'], b['v_mask'] = b['vfeats'][:N][idx].contiguous(), b['v_mask'][:N][idx].contiguous()

            def run(n, first=0):
                with torch.no_grad():
                    for i in range(first, first + n):
                        b = batches[i % nres]
                        _, sl, el = model(b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'])
                        model.extract_index(sl, el)
        elif what == 'B':
            encs = [model.encode_video(b['vfeats'][:N].contiguous(), b['v_mask'][:N].contiguous()) for b in batches]
            for b in batches:
                del b['vfeats']
            idx32 = idx.to(torch.int32)

            def run(n, first=0):
                with torch.no_grad():
                    for i in range(first, first + n):
                        b = batches[i % nres]
                        _, sl, el = model.localize(encs[i % nres], idx32, b['word_ids'], b['char_ids'], b['q_mask'])
                        model.extract_index(sl, el)
        else:
            def run(n, first=0):
                with torch.no_grad():
                    for i in range(first, first + n):
                        b = batches[i % nres]
                        model.encode_video(b['vfeats'], b['v_mask'])
    ms, times, steps = _timed(run, min_region_s, regions)
    eng = model._engine
    eng.profile_select('*')
    run(3)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_select(None)
    ws = {'A': eng.inference_workspace_floats(B, T, LQ, LC), 'B': eng.localize_workspace_floats(B, T, LQ, LC), 'E': eng.encode_workspace_floats(B, T)}[what]
    print(json.dumps({'ms': ms, 'regions_ms': times, 'steps': steps, 'N': N if what != 'E' else B, 'workspace_floats': ws, 'device': torch.cuda.get_device_name(),
                      'per_launch_us': {k: 1e3 * v[0] / v[1] for k, v in prof.items()}, 'launches': {k: v[1] // 3 for k, v in prof.items()}}))


def child_ledger(predictor, B, T, Dv, nres, qpv, out_path):
    """the critical-path ledger (tools/critical_path.py) of ONE localize call in the middle of a back-to-back run, and of one inference forward"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import torch
    from critical_path import ledger
    from vslnet_amd.synthetic import synthetic_batch
    configs, model = _model(predictor, T, Dv)
    N = (B + qpv - 1) // qpv
    batches = [synthetic_batch(configs, B, T, LQ, LC, seed=100 + 1000 * k) for k in range(nres)]
    idx = (torch.arange(B, device='cuda') // qpv).to(torch.int32)
    out = open(out_path, 'w') if out_path else sys.stdout
    with torch.no_grad():
        encs = [model.encode_video(b['vfeats'][:N].contiguous(), b['v_mask'][:N].contiguous()) for b in batches]
        rep = [(b['vfeats'][:N][idx.long()].contiguous(), b['v_mask'][:N][idx.long()].contiguous()) for b in batches]

        def call(which, i):
            b = batches[i % nres]
            if which == 'localize':
                _, sl, el = model.localize(encs[i % nres], idx, b['word_ids'], b['char_ids'], b['q_mask'])
            else:
                _, sl, el = model(b['word_ids'], b['char_ids'], rep[i % nres][0], rep[i % nres][1], b['q_mask'])
            model.extract_index(sl, el)
        for which in ('inference forward on replicated features', 'localize'):
            for i in range(30):
                call(which, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(100):
                call(which, i)
            torch.cuda.synchronize()
            plain = (time.perf_counter() - t0) / 100 * 1e3
            for i in range(30):
                call(which, i)
            eng = model._engine
            eng.profile_select('*')
            for i in range(11):
                call(which, 30 + i)
            torch.cuda.synchronize()
            recs = eng.profile_launches()
            eng.profile_select(None)
            per = len(recs) // 11
            ledger(recs[:per], out, ms_per_step=plain, what='one call (%s)' % which, unit='call',
                   title='critical-path ledger (tools/localize_rate.py --ledger): %s, B=%d T=%d Dv=%d Lq=%d %s, %d queries per video' % (which, B, T, Dv, LQ, predictor, qpv))
            out.write('\n')
    if out_path:
        out.close()
        print(open(out_path).read())


def eval_split(configs):
    """a resident test split with several records per video and ragged video lengths (data.synthetic_dataset makes one video per record)"""
    import numpy as np
    from vslnet_amd.data import ResidentSplit, index_to_time
    rs = np.random.RandomState(17)
    feats, recs = {}, []
    for v in range(EVAL['n_videos']):
        L = EVAL['tmax'] if v == 0 else int(rs.randint(EVAL['tmax'] // 2, EVAL['tmax'] + 1))
        feats['v%03d' % v] = rs.randn(L, EVAL['Dv']).astype(np.float32)
    order = [v for v in range(EVAL['n_videos']) for _ in range(EVAL['per_video'])]
    rs.shuffle(order)
    for v in order:
        L = feats['v%03d' % v].shape[0]
        s = int(rs.randint(0, L - 2))
        e = int(min(L - 1, s + rs.randint(1, max(2, L // 3))))
        dur = float(L) * 1.5
        w = [int(x) for x in rs.randint(2, configs.word_size, size=int(rs.randint(3, LQ + 1)))]
        c = [[2 + (wi * 7 + k) % (configs.char_size - 2) for k in range(1 + wi % 6)] for wi in w]
        st, et = index_to_time(s, e, L, dur)
        recs.append({'sample_id': len(recs), 'vid': 'v%03d' % v, 's_time': float(st), 'e_time': float(et), 'duration': dur,
                     'words': ['w%d' % x for x in w], 's_ind': s, 'e_ind': e, 'v_len': L, 'w_ids': w, 'c_ids': c})
    return ResidentSplit(recs, feats, configs, 'cuda', train=False)


def child_eval(what, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from vslnet_amd import runner
    configs, model = _model('transformer', EVAL['tmax'], EVAL['Dv'])
    configs.batch_size = EVAL['batch']
    split = eval_split(configs)

    def run(n, first=0):
        for _ in range(n):
            if what == 'A':
                runner.eval_test(model, split, 'cuda')
            else:
                runner.eval_test_shared(model, split, 'cuda', videos_per_call=EVAL['batch'])
    run(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(2)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 2
    steps = max(2, int(min_region_s / per) + 1)
    times = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0) / steps)
    rows = int(sum(int(split.lens[a:a + EVAL['batch']].max()) * len(split.lens[a:a + EVAL['batch']]) for a in range(0, len(split.records), EVAL['batch'])))
    print(json.dumps({'ms': statistics.median(times), 'regions_ms': times, 'steps': steps, 'device': torch.cuda.get_device_name(), 'records': len(split.records),
                      'rows_batch_max': rows, 'rows_tmax': len(split.records) * int(split.feats.shape[1]), 'metrics': list(
                          (runner.eval_test if what == 'A' else runner.eval_test_shared)(model, split, 'cuda')[:4])}))


def run_child(args, a, name):
    env = dict(os.environ)          # (VSLNET_HIP_LIB, when set, names the build that is measured)
    cmd = [sys.executable, os.path.abspath(__file__), '--child'] + [str(x) for x in args] + ['--min-region', str(a.min_region), '--regions', str(a.regions)]
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
    ap.add_argument('--child', nargs='+')
    ap.add_argument('--min-region', type=float, default=0.5)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--commit', default=None, help='what the record calls this build (default: git rev-parse of the checkout)')
    ap.add_argument('--only', default=None, help='comma-separated indices into SHAPES; `eval` = the evaluation pass')
    ap.add_argument('--out', default=None)
    ap.add_argument('--ledger', type=int, default=None, help='index into SHAPES: print the critical-path ledger of one inference forward and of one localize call (4 queries per video) instead')
    a = ap.parse_args()
    if a.ledger is not None:
        name, predictor, B, T, Dv, nres = SHAPES[a.ledger]
        child_ledger(predictor, B, T, Dv, nres, 4, a.out)
        return 0
    if a.child:
        if a.child[0] == 'eval':
            child_eval(a.child[1], a.min_region, a.regions)
        else:
            what, predictor, B, T, Dv, nres, qpv = a.child
            child(what, predictor, int(B), int(T), int(Dv), int(nres), int(qpv), a.min_region, a.regions)
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

    def flush():
        if a.out:
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    emit('# %s.  Evaluation calls (model.eval(), no_grad, extract_index included), Lq %d Lc %d, median of %d regions of >= %.1f s, HBM-resident batches rotated'
         % (commit, LQ, LC, a.regions, a.min_region))
    emit('# A = inference forward on the replicated (B, T, Dv) block ; B = localize on a resident (N, T, 128) encoding, N = ceil(B / qpv) ; A / B / A / B, one fresh')
    emit('# process each.  ms are call time per batch of B queries.  encode = encode_video on B videos per call, per video.  break-even = encode / ((A - B) / B)')
    only = None if a.only is None else a.only.split(',')
    shapes = [s for i, s in enumerate(SHAPES) if only is None or str(i) in only]
    rc = 0

    def first_box(out):
        if not lines[0].startswith('# box'):
            lines.insert(0, '# box: ' + out['device'])
    for name, predictor, B, T, Dv, nres in shapes:
        enc, err = run_child(['E', predictor, B, T, Dv, nres, 1], a, name + ' encode')
        if err:
            emit('STOPPED: ' + err)
            flush()
            return 1
        first_box(enc)
        enc_per_video = enc['ms'] / B
        emit('%-30s encode_video: %8.3f ms per call of %d videos = %.4f ms per video   workspace %.3f GiB' % (name, enc['ms'], B, enc_per_video, enc['workspace_floats'] * 4 / 2 ** 30))
        top = sorted(enc['per_launch_us'].items(), key=lambda kv: -kv[1] * enc['launches'][kv[0]])[:5]
        emit('    encode per launch: ' + '  '.join('%s %.1f us x %d' % (k, v, enc['launches'][k]) for k, v in top))
        for qpv in QPV:
            res = {'A': [], 'B': []}
            for which in ('A', 'B', 'A', 'B'):
                out, err = run_child([which, predictor, B, T, Dv, nres, qpv], a, '%s qpv %d %s' % (name, qpv, which))
                if err:
                    emit('STOPPED: ' + err)
                    flush()
                    return 1
                res[which].append(out)
            am, bm = [o['ms'] for o in res['A']], [o['ms'] for o in res['B']]
            A, Bm, spread = statistics.mean(am), statistics.mean(bm), abs(am[0] - am[1])
            ok = A - Bm > spread
            saving = (A - Bm) / B
            emit('%-30s qpv %2d (N %2d)  A %8.3f %8.3f ms  B %8.3f %8.3f ms  spread(A) %6.3f ms  B/A %.3f  saving %.4f ms per query  break-even %s queries per video  '
                 'workspace %.3f -> %.3f GiB  %s' % (name, qpv, res['B'][0]['N'], am[0], am[1], bm[0], bm[1], spread, Bm / A, saving,
                                                    ('%.2f' % (enc_per_video / saving)) if saving > 0 else 'none', res['A'][0]['workspace_floats'] * 4 / 2 ** 30,
                                                    res['B'][0]['workspace_floats'] * 4 / 2 ** 30, 'ok' if ok else 'DEFECT'))
            rc = rc or (0 if ok else 3)
            if qpv == QPV[0]:
                for which in ('A', 'B'):
                    o = res[which][0]
                    top = sorted(o['per_launch_us'].items(), key=lambda kv: -kv[1] * o['launches'][kv[0]])[:9]
                    emit('    %s per launch: ' % which + '  '.join('%s %.1f us x %d' % (k, v, o['launches'][k]) for k, v in top))
            flush()
    if only is None or 'eval' in only:
        res = {'A': [], 'B': []}
        for which in ('A', 'B', 'A', 'B'):
            out, err = run_child(['eval', which], a, 'evaluation pass ' + which)
            if err:
                emit('STOPPED: ' + err)
                flush()
                return 1
            first_box(out)
            res[which].append(out)
        o = res['A'][0]
        am, bm = [x['ms'] for x in res['A']], [x['ms'] for x in res['B']]
        emit('# one evaluation pass, %d records over %d videos (%d per video), ragged lengths up to %d clips, Dv %d, batches of %d: eval_test pads a batch to its own '
             'maximum (%d rows in all), eval_test_shared to the longest video (%d rows) and includes encoding the %d videos.  Reported, not gated.'
             % (o['records'], EVAL['n_videos'], EVAL['per_video'], EVAL['tmax'], EVAL['Dv'], EVAL['batch'], o['rows_batch_max'], o['rows_tmax'], EVAL['n_videos']))
        emit('evaluation pass                eval_test %8.3f %8.3f ms  eval_test_shared %8.3f %8.3f ms  shared / plain %.3f   metrics %s | %s'
             % (am[0], am[1], bm[0], bm[1], statistics.mean(bm) / statistics.mean(am), ['%.2f' % m for m in res['A'][0]['metrics']], ['%.2f' % m for m in res['B'][0]['metrics']]))
    flush()
    return rc


if __name__ == '__main__':
    sys.exit(main())
