"""What the video ranking loss costs a training step: the shared step with the lazy fused loss on the PARENT library (A) against the same step with
Engine.group_loss (B), same box.  It records; it does not promise.

    python tools/build_base.py <parent> base                       # A's library: the parent commit
    python tools/rank_loss_rate.py [--out profiles/rank_loss_rate.txt] [--base vslnet_amd/lib/libvslnet_hip_base.so]

The step: configs[1]'s model (transformer predictor, Dv 1024, T 128), 64 pair rows over 16 videos -- 16 queries, each against its own video and
n = 3 others, the groups of ResidentSplit.shards(negatives=3).  A = forward_shared, loss(lazy=True) -- the loss launch rides behind the backward's
chain --, backward with the fused AdamW step, on the parent library.  B = this build: forward_shared, group_loss (two launches of its own in front
of the backward: the loss is back on the dependent chain), the same backward call.  A / B / A / B, every measurement a fresh child process under
its own time limit; the script stops at the first child that does not exit with 0.  A child rotates HBM-resident batches, warms up, sizes a region
to at least 0.5 s, times five device-synchronised regions and reports their median.  The spread is the difference between the two A runs.  Also
reported from the launch ledger: the two group-loss kernels' own times in B and the `loss` launch's in A."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, VIDEOS, NEG, T, DV, LQ, LC, NRES = 64, 16, 3, 128, 1024, 20, 10, 10


def child(what, min_region_s, regions):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from vslnet_amd.dp import FlatAdamW, backward_exchange_step
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.synthetic import make_configs, synthetic_batch
    configs = make_configs(video_feature_dim=DV, max_pos_len=T, drop_rate=0.2, predictor='transformer')
    torch.manual_seed(configs.seed)
    model = VSLNet(configs, torch.randn(configs.word_size - 2, configs.word_dim).numpy()).cuda().train()
    flat, grads = model.flat_parameters
    eng = model._engine
    pad_vec, glove_vec = model.embedding_net.word_emb.pad_vec.data, model.embedding_net.word_emb.glove_vec.data
    G = ROWS // (1 + NEG)                                              # 16 queries = 16 videos: the query of group g owns video g
    rs = np.random.RandomState(0)
    vid = np.concatenate([[g] + list(rs.permutation([v for v in range(VIDEOS) if v != g])[:NEG]) for g in range(G)])
    query = np.repeat(np.arange(G), 1 + NEG)
    d_vid, d_query = torch.from_numpy(vid).cuda(), torch.from_numpy(query).cuda()
    idx32 = d_vid.to(torch.int32)
    group_start = torch.arange(0, ROWS + 1, 1 + NEG, dtype=torch.int32).cuda()
    positive = group_start[:-1].contiguous()
    is_pos = torch.zeros(ROWS, dtype=torch.int64).cuda()
    is_pos[positive.long()] = 1
    batches = [synthetic_batch(configs, ROWS, T, LQ, LC, seed=100 + 1000 * k) for k in range(NRES)]
    for b in batches:
        b['video_v_mask'], b['vfeats'] = b['v_mask'][:VIDEOS].contiguous(), b['vfeats'][:VIDEOS].contiguous()
        b['v_mask'] = b['video_v_mask'][d_vid].contiguous()
        for k in ('word_ids', 'char_ids', 'q_mask'):
            b[k] = b[k][d_query].contiguous()
        b['s_labels'], b['e_labels'] = b['s_labels'][d_query] * is_pos, b['e_labels'][d_query] * is_pos
        b['h_labels'] = (b['h_labels'][d_query] * is_pos[:, None]).contiguous()
    mask_sum = float(batches[0]['v_mask'].sum().item())
    opt = FlatAdamW(flat, eng.layout, lr=configs.init_lr, num_train_steps=10 ** 7, clip_norm=configs.clip_norm, engine=eng)

    def run(n, first=0):
        for i in range(first, first + n):
            b = batches[i % NRES]
            eng.forward_shared(flat, pad_vec, glove_vec, b['word_ids'], b['char_ids'], b['vfeats'], b['video_v_mask'], b['q_mask'], idx32, training=True, seed=i)
            if what == 'B':
                _, _, _, d_h, d_sl, d_el = eng.group_loss(b['s_labels'], b['e_labels'], b['h_labels'], group_start, positive, 1.0, configs.highlight_lambda, 1.0,
                                                          0.1, 'max', inv_pos=1.0 / G, inv_groups=1.0 / G, mask_sum=mask_sum)
            else:
                _, d_h, d_sl, d_el = eng.loss(b['s_labels'], b['e_labels'], b['h_labels'], 1.0, configs.highlight_lambda, inv_batch=1.0 / ROWS, mask_sum=mask_sum, lazy=True)
            backward_exchange_step(eng, None, grads, (d_h, d_sl, d_el), opt)
    run(5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(5)
    torch.cuda.synchronize()
    steps = max(5, int(min_region_s / ((time.perf_counter() - t0) / 5)) + 1)
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
    print(json.dumps({'ms': statistics.median(times), 'steps': steps, 'device': torch.cuda.get_device_name(), 'finite': bool(torch.isfinite(flat).all()),
                      'per_launch_us': {k: 1e3 * v[0] / v[1] for k, v in prof.items()}}))


def run_child(what, a):
    env = dict(os.environ)
    env.pop('VSLNET_HIP_LIB', None)
    if what == 'A':
        env['VSLNET_HIP_LIB'] = os.path.abspath(a.base)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', what, '--min-region', str(a.min_region), '--regions', str(a.regions)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        return None, '%s: child timed out after %d s' % (what, a.child_timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    if r.returncode != 0 or not lines:
        return None, '%s: child exit status %d: %s' % (what, r.returncode, (r.stderr.strip().splitlines() or [''])[-1])
    out = json.loads(lines[-1])
    return (out, None) if out['finite'] else (None, '%s: parameters not finite after the run' % what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None)
    ap.add_argument('--min-region', type=float, default=0.5)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--child-timeout', type=int, default=120)
    ap.add_argument('--base', default=os.path.join(ROOT, 'vslnet_amd', 'lib', 'libvslnet_hip_base.so'), help="the parent commit's library (tools/build_base.py)")
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.min_region, a.regions)
        return 0
    if not os.path.exists(a.base):
        print('no parent library at %s: build it with tools/build_base.py <parent> base' % a.base, file=sys.stderr)
        return 2
    lines, res = [], {'A': [], 'B': []}

    def emit(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
        if a.out:
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    emit('# Shared training step, transformer predictor, %d pair rows over %d videos (n = %d negatives per query), T %d Dv %d Lq %d Lc %d, drop_rate 0.2,'
         % (ROWS, VIDEOS, NEG, T, DV, LQ, LC))
    emit('# median of %d regions of >= %.1f s.  A = the parent library, lazy fused loss ; B = this build, group_loss (2 launches in front of the backward).' % (a.regions, a.min_region))
    for which in ('A', 'B', 'A', 'B'):
        out, err = run_child(which, a)
        if err:
            emit('STOPPED: ' + err)
            return 1
        res[which].append(out)
    emit('# box: ' + res['A'][0]['device'])
    am, bm = [o['ms'] for o in res['A']], [o['ms'] for o in res['B']]
    spread = abs(am[0] - am[1])
    verdict = 'faster' if max(bm) < min(am) - spread else 'slower' if min(bm) > max(am) + spread else 'inside the spread of A'
    emit('A %8.4f %8.4f ms per step   spread(A) %.4f ms' % (am[0], am[1], spread))
    emit('B %8.4f %8.4f ms per step   B - A %+.4f ms  B/A %.4f  %s' % (bm[0], bm[1], statistics.mean(bm) - statistics.mean(am), statistics.mean(bm) / statistics.mean(am), verdict))
    pa, pb = res['A'][0]['per_launch_us'], res['B'][0]['per_launch_us']
    emit('kernels alone (launch ledger, us): A loss %.2f ; B group_loss_a %.2f + group_loss_c %.2f = %.2f'
         % (pa.get('loss', float('nan')), pb.get('group_loss_a', float('nan')), pb.get('group_loss_c', float('nan')),
            pb.get('group_loss_a', float('nan')) + pb.get('group_loss_c', float('nan'))))
    emit('# B - A above is what putting the loss back on the dependent chain costs this step (the two kernels and their launch gaps between the forward\'s last')
    emit('# kernel and the backward\'s first), beyond the ranking term itself.')
    return 0


if __name__ == '__main__':
    sys.exit(main())
