"""Gradient accumulation: pairs/s of ONE accumulated optimizer step (K micro-batches into one bucket, clip + AdamW on the sum behind the last one)
against K plain steps of the micro size with the same library -- what the accumulation itself costs: one read of the bucket per reduction, K - 1
optimizer updates fewer.  Dv=1024, Lq=20, Lc=10, transformer, 8 heads, drop 0.2, train mode, the production sequence (lazy loss, fused step):

    T=256   global batch 1024 as K=16 x 64 and as K=32 x 32      (BASELINE configs[3]'s global batch: its training plan does not fit one workspace)
    T=4096  global batch 64 as K=4 x 16                          (the largest micro-batch that fits at that length)

Every case runs in a fresh child process under its own time limit; inside it the two forms alternate, region by region:

    python tools/accum_rate.py [--steps 5] [--regions 3] [--out profiles/accum_rate.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(256, 1024, 16), (256, 1024, 32), (4096, 64, 4)]          # T, global batch, K


def child(T, B, K, steps, regions):
    sys.path.insert(0, ROOT)
    import torch
    from vslnet_amd import dp
    from vslnet_amd.engine import VslError
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.synthetic import make_configs, synthetic_batch
    configs = make_configs(video_feature_dim=1024, max_pos_len=T, drop_rate=0.2, predictor='transformer', num_heads=8)
    torch.manual_seed(0)
    glove = torch.randn(configs.word_size - 2, configs.word_dim).numpy()
    model = VSLNet(configs, glove).cuda().train()
    flat, grads = model.flat_parameters
    eng = model._engine
    out = {'T': T, 'B': B, 'K': K, 'accumulation': bool(eng.has_grad_accumulation)}
    try:
        eng.workspace_floats(B, T, 20, 10)
        out['global_plan'] = 'fits'
    except VslError as e:
        out['global_plan'] = 'refused: ' + str(e)
    cuts = dp.micro_slices(B, K)
    out['micro_workspace_floats'] = eng.workspace_floats(cuts[0].stop - cuts[0].start, T, 20, 10)
    b = synthetic_batch(configs, B, T, 20, 10, seed=1, ragged=True)
    pieces = [{k: v[c].contiguous() for k, v in b.items()} for c in cuts]
    del b
    pad_vec, glove_vec = model.embedding_net.word_emb.pad_vec.data, model.embedding_net.word_emb.glove_vec.data
    msums = [float(p['v_mask'].sum()) for p in pieces]
    msum = sum(msums)
    opt = dp.FlatAdamW(flat, eng.layout, lr=1e-4, num_train_steps=10 ** 6, engine=eng)

    def forward_loss(p, seed, row0, inv_batch, mask_sum):
        eng.forward(flat, pad_vec, glove_vec, p['word_ids'], p['char_ids'], p['vfeats'], p['v_mask'], p['q_mask'], training=True, seed=seed, sample_offset=row0)
        return eng.loss(p['s_labels'], p['e_labels'], p['h_labels'], 1.0, 5.0, inv_batch=inv_batch, mask_sum=mask_sum, lazy=True)[1:]

    def accumulated(i):         # ONE optimizer step over the K pieces of the global batch
        for j, (p, c) in enumerate(zip(pieces, cuts)):
            dp.backward_exchange_step(eng, None, grads, forward_loss(p, i, c.start, 1.0 / B, msum), opt, accumulate=j > 0, update=j == K - 1)

    def plain(i):               # K optimizer steps, one per piece: a batch of the micro size each
        for j, p in enumerate(pieces):
            dp.backward_exchange_step(eng, None, grads, forward_loss(p, i * K + j, 0, 1.0 / p['vfeats'].shape[0], msums[j]), opt)
    for fn in (accumulated, plain):
        fn(0)
    torch.cuda.synchronize()
    times = {'accumulated': [], 'plain': []}
    for r in range(regions):
        for name, fn in (('accumulated', accumulated), ('plain', plain)):
            t0 = time.perf_counter()
            for i in range(steps):
                fn(100 + r * steps + i)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / steps)
    eng.profile_select('adamw,reduce')
    accumulated(1000)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_select(None)
    out['ms'] = {k: statistics.median(v) for k, v in times.items()}
    out['ms_all'] = times
    out['ledger_us'] = {k: [1e3 * v[0] / v[1], v[1]] for k, v in prof.items()}
    out['finite'] = bool(torch.isfinite(flat).all())
    print(json.dumps(out))


def run(T, B, K, steps, regions, timeout=600):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', str(T), str(B), str(K), '--steps', str(steps), '--regions', str(regions)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {'error': 'timeout'}, True
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    if r.returncode != 0 or not lines:
        fatal = r.returncode < 0 or r.returncode in (134, 139)          # a fault: start nothing more on the GPU
        return {'error': 'rc %d: %s' % (r.returncode, r.stderr.strip().splitlines()[-1:] if r.stderr else '')}, fatal
    return json.loads(lines[-1]), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', nargs=3, type=int)
    ap.add_argument('--steps', type=int, default=5, help='accumulated steps (and groups of K plain steps) per timed region')
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.child[2], a.steps, a.regions)
        return
    lines = []

    def emit(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
    import torch
    emit('device: %s   median of %d regions x %d accumulated steps (alternating with %d x K plain steps), train mode, drop 0.2, Dv=1024 Lq=20 Lc=10, '
         'transformer, 8 heads, lazy loss + fused step' % (torch.cuda.get_device_name(), a.regions, a.steps, a.steps))
    del torch
    for T, B, K in CASES:
        res, fatal = run(T, B, K, a.steps, a.regions)
        tag = 'T=%-5d global batch %-5d K=%-3d x %-3d' % (T, B, K, B // K)
        if 'error' in res:
            emit('%s error: %s' % (tag, res['error']))
        else:
            acc, pl = res['ms']['accumulated'], res['ms']['plain']
            emit('%s one accumulated step %9.3f ms = %8.1f pairs/s | %d plain steps of %d: %9.3f ms = %8.1f pairs/s | accumulated / plain = %.4f'
                 % (tag, acc, B / (acc / 1e3), K, B // K, pl, B / (pl / 1e3), acc / pl))
            emit('    regions (ms): accumulated %s | plain %s' % (' '.join('%.3f' % x for x in res['ms_all']['accumulated']),
                                                               ' '.join('%.3f' % x for x in res['ms_all']['plain'])))
            emit('    the global batch as one step: %s' % res['global_plan'].split(':')[0] + ('' if res['global_plan'] == 'fits' else ' (' + res['global_plan'].split(': ', 2)[-1] + ')'))
            emit('    micro-batch workspace %d floats (%.2f GiB); ledger of one accumulated step: %s; parameters finite: %s'
                 % (res['micro_workspace_floats'], res['micro_workspace_floats'] * 4 / 2 ** 30,
                    '  '.join('%s %.1f us x %d' % (k, v[0], v[1]) for k, v in sorted(res['ledger_us'].items())), res['finite']))
        if fatal:
            break
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
