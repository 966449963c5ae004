"""Localising in one long video by sliding windows: what a user can do with the parent library (A) beside encode_windows + localize_long (B).

    python tools/build_base.py <parent>                 # vslnet_amd/lib/libvslnet_hip_base.so
    python tools/window_rate.py [--out profiles/window_rate.txt] [--commit <hash>]

A (the base library, which has neither vsl_encode_windows nor vsl_merge_windows):
    1. unfold the features into the (W, T, Dv) block of overlapping windows (zero-padded last window) ; 2. encode_video on it, `--windows-per-call` at a time ;
    3. localize_pairs of every (window, query), `--pairs-per-call` at a time ; 4. extract_topk per list ; 5. the lists to the host, the NMS merge in numpy
    (vslnet_amd.spans.merge_windows_reference).
B (this build): encode_windows + localize_long with the same chunk sizes.

Per shape four fresh child processes, A / B / A / B, each under its own time limit; the script stops at the first child that does not exit with 0.  A child
builds the module and the data, warms every item up once and then measures each `--repeat` times as a device-synchronised region: the two encodes, the
localize + extract part, the two merges (A's includes its device-to-host copy), the whole call, and the peak of torch's allocator over one whole call.
The record prints both values of each variant and B / A of their means.  Nothing here is a gate: the record states what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = os.path.join(ROOT, 'vslnet_amd', 'lib', 'libvslnet_hip_base.so')
#          clips   Dv  window stride queries k
SHAPES = [(16384, 1024, 128, 64, 64, 5), (16384, 1024, 128, 32, 64, 5)]
LQ, LC, NMS = 12, 8, 0.5


def child(variant, L, Dv, window, stride, Q, k, repeat, per_enc, per_pairs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd.spans import merge_windows_reference, window_table
    from vslnet_amd.synthetic import make_configs, synthetic_batch
    configs = make_configs(video_feature_dim=Dv, max_pos_len=window, predictor='transformer')
    torch.manual_seed(configs.seed)
    model = VSLNet(configs, torch.randn(configs.word_size - 2, configs.word_dim).numpy()).cuda().eval()
    assert model._engine_for(torch.device('cuda')).has_windows == (variant == 'B'), 'A runs the base library, B this build'
    qb = synthetic_batch(configs, Q, 8, LQ, LC, seed=100, ragged=True)
    feats = torch.randn(L, Dv, device='cuda')
    start, length = window_table(L, window, stride)
    W = len(start)
    d_len = torch.from_numpy(length.astype(np.int32)).cuda()
    widx = torch.arange(W, dtype=torch.int32, device='cuda').repeat_interleave(Q)      # list b = window b // Q, query b % Q ; group = the query
    qidx = torch.arange(Q, dtype=torch.int32, device='cuda').repeat(W)

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    with torch.no_grad():
        qenc = model.encode_query(qb['word_ids'], qb['char_ids'], qb['q_mask'])

        def encode_a():
            from vslnet_amd.engine import VideoEncoding
            pad = (W - 1) * stride + window - L
            x = torch.cat([feats, feats.new_zeros(pad, Dv)]) if pad else feats
            block = x.unfold(0, window, stride).permute(0, 2, 1).contiguous()            # (W, T, Dv): the replicated block
            mask = (torch.arange(window, device='cuda')[None, :] < d_len[:, None]).float()
            enc, part = torch.empty(W, window, 128, device='cuda'), None
            for a in range(0, W, per_enc):
                part = model.encode_video(block[a:a + per_enc], mask[a:a + per_enc])
                enc[a:a + per_enc] = part.encoding
            return VideoEncoding(enc, mask, owner=part.owner, epoch=part.epoch)

        def lists_a(venc):
            out = []
            for a in range(0, W * Q, per_pairs):
                _, sl, el = model.localize_pairs(venc, qenc, widx[a:a + per_pairs], qidx[a:a + per_pairs])
                out.append(model.extract_topk(sl, el, k, nms_iou=NMS, lengths=d_len[widx[a:a + per_pairs].long()], want_prob=True))
            return out

        def merge_a(lists):
            host = [torch.cat([getattr(s, n) for s in lists]).cpu().numpy() for n in ('start', 'end', 'score', 'prob', 'count')]
            return merge_windows_reference(*host, qidx.cpu().numpy(), Q, k, NMS, np.repeat(start, Q))

        def whole_a():
            return merge_a(lists_a(encode_a()))

        def encode_b():
            return model.encode_windows(feats, window, stride, windows_per_call=per_enc)

        def whole_b():
            return model.localize_long(encode_b(), qenc, k, nms_iou=NMS, pairs_per_call=per_pairs)

        rec = {'variant': variant, 'windows': W, 'lists': W * Q}
        if variant == 'A':
            venc = encode_a()
            lists = lists_a(venc)
            merge_a(lists)
            items = [('encode', encode_a), ('localize+extract', lambda: lists_a(venc)), ('merge', lambda: merge_a(lists)), ('whole', whole_a)]
            whole = whole_a
        else:
            from vslnet_amd.engine import TopkSpans
            wenc = encode_b()
            whole_b()
            eng = model._engine
            lists = lists_a(wenc)                                                        # (the same lists, for the merge alone)
            spans = TopkSpans(*(torch.cat([getattr(s, n) for s in lists]).contiguous() for n in ('start', 'end', 'score', 'prob', 'count')))
            off = wenc.offset_of_window[widx.long()].contiguous()
            items = [('encode', encode_b), ('localize+extract', lambda: lists_a(wenc)), ('merge', lambda: eng.merge_windows(spans, qidx, Q, k, offset=off, nms_iou=NMS)),
                     ('whole', whole_b)]
            whole = whole_b
        for name, fn in items:
            rec[name] = min(sync_time(fn)[1] for _ in range(repeat))
        del lists
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        whole()
        torch.cuda.synchronize()
        rec['peak_gib'] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    print('RECORD ' + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'window_rate.txt'))
    ap.add_argument('--commit', default='')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--windows-per-call', type=int, default=256)
    ap.add_argument('--pairs-per-call', type=int, default=4096)
    ap.add_argument('--limit', type=int, default=240, help='seconds per child process')
    ap.add_argument('--child', nargs=7)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], *(int(x) for x in a.child[1:]), a.repeat, a.windows_per_call, a.pairs_per_call)
        return
    if not os.path.exists(BASE):
        sys.exit('%s is missing: python tools/build_base.py <parent>' % BASE)
    lines = ['# one video by sliding windows, Lq %d Lc %d, k and nms_iou %.1f as given; A = the parent library (unfold + encode_video + localize_pairs + extract_topk +'
             % (LQ, LC, NMS), '# copy + numpy merge), B = %s (encode_windows + localize_long); A / B / A / B, one fresh process each; ms = the best of %d'
             % (a.commit or 'this build', a.repeat), '# device-synchronised calls; chunks of %d windows / %d pairs; peak = torch allocator over one whole call'
             % (a.windows_per_call, a.pairs_per_call)]
    for shape in SHAPES:
        recs = {'A': [], 'B': []}
        for variant in 'ABAB':
            env = dict(os.environ)
            if variant == 'A':
                env['VSLNET_HIP_LIB'] = BASE
            else:
                env.pop('VSLNET_HIP_LIB', None)
            cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--repeat', str(a.repeat), '--windows-per-call',
                   str(a.windows_per_call), '--pairs-per-call', str(a.pairs_per_call), '--child', variant] + [str(x) for x in shape]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit('child %s %s exited with %d: stopping' % (variant, shape, r.returncode))
            recs[variant].append(json.loads([x for x in r.stdout.split('\n') if x.startswith('RECORD ')][-1][7:]))
        L, Dv, window, stride, Q, k = shape
        lines.append('clips %d Dv %d window %d stride %d: %d windows x %d queries = %d lists, k %d' % (L, Dv, window, stride, recs['A'][0]['windows'], Q, recs['A'][0]['lists'], k))
        for name in ('encode', 'localize+extract', 'merge', 'whole', 'peak_gib'):
            va, vb = [r[name] for r in recs['A']], [r[name] for r in recs['B']]
            unit = 'GiB' if name == 'peak_gib' else 'ms'
            lines.append('    %-17s A %9.3f %9.3f %s   B %9.3f %9.3f %s   B/A %.3f' % (name, va[0], va[1], unit, vb[0], vb[1], unit, sum(vb) / sum(va)))
        print('\n'.join(lines[-6:]), flush=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
