"""Call time of `extract_topk` (the K best moments per query, greedy temporal NMS) beside what it is compared with, on the same logits:

    (a) `extract_index`, the one-span kernel;
    (b) the torch composition a user would write without the call and WITHOUT NMS: outer sum, triu mask, topk on the flattened (B, T T) tensor
        (only where that tensor fits: --max-square-gib);
    (c) the inference forward of the shape, for scale.

    python tools/topk_rate.py [--out profiles/topk_rate.txt] [--commit <hash>]

Per shape two fresh child processes, A and A', one after the other, each under its own time limit; the script stops at the first child that does not
exit with 0.  A child builds the module, runs the inference forward of one synthetic batch to get logits as the model emits them (ragged masks), and then
measures every item twice in alternation (item 1, item 2, ..., item 1, item 2, ...): warm-up, a region sized to at least --min-region seconds, the
time per call of that device-synchronised region.  The record prints, per item, the mean of the four values and their spread (max - min over both
rounds of both processes).  Nothing here is a gate: the record states what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 128), (32, 256), (64, 1024), (16, 4096)]       # (B, T)
KS, NMS = (1, 5, 10), (1.0, 0.5)
LQ, LC, DV = 20, 10, 1024


def child(B, T, min_region_s, max_square_gib):
    sys.path.insert(0, ROOT)
    import torch
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.synthetic import make_configs, synthetic_batch
    configs = make_configs(video_feature_dim=DV, max_pos_len=max(T, LQ), predictor='transformer')
    torch.manual_seed(configs.seed)
    model = VSLNet(configs, torch.randn(configs.word_size - 2, configs.word_dim).numpy()).cuda().eval()
    b = synthetic_batch(configs, B, T, LQ, LC, seed=100, ragged=True)

    def forward():
        return model(b['word_ids'], b['char_ids'], b['vfeats'], b['v_mask'], b['q_mask'])
    with torch.no_grad():
        _, sl, el = forward()
    sl, el = sl.clone(), el.clone()
    lengths = b['v_mask'].sum(dim=1).to(torch.int32)
    lower = ~torch.triu(torch.ones(T, T, dtype=torch.bool, device='cuda'))

    def torch_topk():       # no NMS, no lengths beyond the logits' own mask: the least a host-side version has to do (no host-to-device copy inside)
        sq = (sl[:, :, None] + el[:, None, :]).masked_fill_(lower, float('-inf'))
        v, i = torch.topk(sq.view(B, T * T), 5, dim=1)
        return v, i // T, i % T
    items = [('extract_topk K %2d nms %.1f' % (k, n), (lambda k=k, n=n: model.extract_topk(sl, el, k, nms_iou=n, lengths=lengths))) for k in KS for n in NMS]
    items.append(('(a) extract_index', lambda: model.extract_index(sl, el)))
    if B * T * T * 4 <= max_square_gib * 2 ** 30:
        items.append(('(b) torch outer sum + triu + topk 5', torch_topk))
    items.append(('(c) inference forward', forward))
    out = {name: [] for name, _ in items}
    with torch.no_grad():
        for rnd in range(2):
            for name, fn in items:
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
                out[name].append(1e6 * (time.perf_counter() - t0) / n)
    print(json.dumps({'us': out, 'device': torch.cuda.get_device_name(), 'mean_len': float(lengths.float().mean())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', nargs=2)
    ap.add_argument('--min-region', type=float, default=0.3)
    ap.add_argument('--max-square-gib', type=float, default=4.0, help='(b) runs only where the (B, T, T) fp32 tensor is at most this large')
    ap.add_argument('--child-timeout', type=int, default=150)
    ap.add_argument('--commit', default=None, help='what the record calls this build (default: git rev-parse of the checkout)')
    ap.add_argument('--only', default=None, help='comma-separated indices into SHAPES')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), a.min_region, a.max_square_gib)
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
    emit('# extract_topk call time (%s), logits of the inference forward of a synthetic batch (ragged lengths), Lq %d Lc %d Dv %d; us per call of a device-synchronised'
         % (commit, LQ, LC, DV))
    emit('# region of >= %.1f s; per item: mean of 2 rounds x 2 fresh processes (A, A\'), spread = max - min of those four.  (b) has no NMS and K = 5.' % a.min_region)
    for B, T in (SHAPES if a.only is None else [SHAPES[int(i)] for i in a.only.split(',')]):
        runs = []
        for _ in range(2):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', str(B), str(T), '--min-region', str(a.min_region), '--max-square-gib', str(a.max_square_gib)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                emit('STOPPED: B %d T %d: child timed out after %d s' % (B, T, a.child_timeout))
                return 1
            js = [l for l in r.stdout.splitlines() if l.startswith('{')]
            if r.returncode != 0 or not js:
                emit('STOPPED: B %d T %d: child exit status %d: %s' % (B, T, r.returncode, (r.stderr.strip().splitlines() or [''])[-1]))
                return 1
            runs.append(json.loads(js[-1]))
        emit('B %d T %d (mean valid length %.0f) on %s; (B, T, T) fp32 = %.3f GiB' % (B, T, runs[0]['mean_len'], runs[0]['device'], B * T * T * 4 / 2 ** 30))
        for name in runs[0]['us']:
            v = runs[0]['us'][name] + runs[1]['us'][name]
            emit('    %-38s %10.1f us   spread %8.1f us   (%s)' % (name, sum(v) / len(v), max(v) - min(v), ' '.join('%.1f' % x for x in v)))
        if not any(n.startswith('(b)') for n in runs[0]['us']):
            emit('    (b) not run: the (B, T, T) tensor exceeds %.1f GiB' % a.max_square_gib)
    return 0


if __name__ == '__main__':
    sys.exit(main())
