"""Did a change of the HOST code (vslnet_amd/csrc: api / layout / plan / streams / forward / backward) change anything a caller can observe?

    VSLNET_HIP_LIB=vslnet_amd/lib/libvslnet_hip_base.so python tools/host_equivalence.py dump base.json      # tools/build_base.py <rev> base
    python tools/host_equivalence.py dump new.json
    python tools/host_equivalence.py diff base.json new.json          # prints every difference; exit status 1 on any

`dump` runs seeded synthetic batches against whichever library VSLNET_HIP_LIB selects and records per case
  * the launch ledger of the call(s) as (name, stream index, dependencies) from Engine.profile_launches() -- timestamps dropped;
  * the four workspace sizes of the shape and vsl_workspace_offset of every name it knows;
  * SHA-256 of every output: h_score, both logits, the extracted indices, the losses, the gradient bucket, and parameters + both moments
    after the fused optimizer step of that backward.
Cases: every row of tests/test_dispatch_boundaries.py::ROWS as one training step (dropout on, fixed seed, fused optimizer step) and as an
inference forward; the smallest shapes that reach the attention kernels those rows do not (1 and 2 heads with the element hash, the pair hash
over two dQ slabs and query-major dQ; 4 and 16 heads with query-major dQ); encode_video + localize with a repeated and permuted video index, both predictors, fp32 and bf16 features;
one training step through a shared encoding (Engine.forward_shared) with the same index, both predictors, at the two shapes that reach the
sample-local and the row-tile query path and the folded and the unfolded CQ column; the headline bench shape; one B > 80 rnn shape (chunked LSTM launches over three streams);
the launchers those do not reach, at B = 3, T = 40, Lq = 9, Dv = 64 unless named: a step with the trainable word table (k_word_table_bwd, k_zero4, the table
branch of embed_fwd), a step on bf16 features (k_vproj_fwd_bf16), the separate calls (an eager loss() that leaves the mask sum to the device, a
loss(want_grads=False), a plain backward(), adamw_step with and without norm_from_backward and the norm it reports), a step at char_dim 100 and
word_dim 52 with Lq = 40 (two channel blocks in the embedding kernels; k_linear_fwd), and a step at Lq = 100, T = 64 (k_cq_score<16>, the
CQ_BIG_LQ layout of k_cq_out and of the CQ backward, the unfolded column).  The whole set runs three times, each in a fresh child process
(the switches are read once per process): default, VSL_MULTI_STREAM=0, and every fusion switch off.  The children run one after the other,
each under its own time limit; the tool stops at the first one that does not exit with 0."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {
    'default': {},
    'single_stream': {'VSL_MULTI_STREAM': '0'},
    'unfused': {'VSL_QKV_FUSED': '0', 'VSL_HEADS_FUSED': '0', 'VSL_QUERY_FUSED': '0', 'VSL_CQ_FOLD': '0', 'VSL_LOSS_INLINE': '0'},
}
ENC = ('venc', 'qenc', 'p1', 'p2')
OFFSET_NAMES = ['video_affine', 'embedding_net', 'emb_concat', 'venc', 'qenc', 'venc_x0', 'venc_conv0', 'venc_conv3', 'venc_q', 'venc_k', 'venc_v', 'venc_att',
                'venc_r', 'qenc_conv3', 'qenc_att', 'cq_score', 'cq_srow', 'cq_scol', 'cq_M', 'cq_attention', 'cq_concat', 'gated', 'pred_s', 'pred_e',
                'd_gated_enc', 'd_gated_hs', 'd_gated_he', 'd_venc', 'd_qenc', 'd_video_affine', 'd_embedding_net', 'd_pred_s', 'd_pred_s_head',
                'd_cq_concat', 'd_cq_attention', 'd_emb_concat', 'hid_s', 'hid_e', 'no_such_name'] + \
               ['relu_%s_%d' % (e, i) for e in ENC for i in range(4)] + ['%s_y%d' % (e, i) for e in ENC for i in range(4)] + ['%s_x0' % e for e in ENC]
SHARED_OFFSET_NAMES = ['d_venc_video', 'group_start', 'group_members']      # vsl_shared_workspace_offset only
STEP_SEED = (5 << 33) + 2024
# (B, T, Lq) beyond test_dispatch_boundaries.ROWS: T = 129 element hash, 257 pair hash + two dQ slabs, 1025 query-major dQ (the DQ = false instantiations)
ATTN_SHAPES_LONG = ((1, 1025, 9),)
ATTN_SHAPES_WIDE = ((2, 129, 9), (2, 257, 9)) + ATTN_SHAPES_LONG


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def ledger(eng):
    return [[r['name'], r['stream'], r['deps']] for r in eng.profile_launches()]


def setup(cfgkw, B, T, Lq, Lc, ragged_extreme=False):
    import torch  # noqa: F401
    from oracle import vslnet_oracle as O
    from tests.helpers import extreme_ragged
    from vslnet_amd.engine import Engine, flat_from_state_dict
    kw = dict(max_pos_len=max(T, Lq), word_size=102, drop_rate=0.2)
    kw.update(cfgkw)
    cfg = O.make_cfg(**kw)
    P = O.random_params(cfg, seed=301)
    b = O.synthetic_batch(cfg, B, T, Lq, Lc, seed=302, ragged=True)
    if ragged_extreme:
        b = extreme_ragged(b)
    d = {k: v.cuda().contiguous() for k, v in b.items()}
    eng = Engine(cfg)
    flat = flat_from_state_dict(eng, P)
    pad, glove = P.get('embedding_net.word_emb.pad_vec'), P.get('embedding_net.word_emb.glove_vec')       # (absent: trainable word table)
    pad, glove = (None if pad is None else pad.cuda()), (None if glove is None else glove.cuda())
    return eng, flat, pad, glove, b, d


def sizes_and_offsets(eng, B, T, Lq, Lc):
    """(after a training forward: vsl_workspace_offset refuses everything after an inference forward)"""
    import ctypes as C
    eng.lib.vsl_workspace_offset.restype = C.c_int64
    out = {'workspace_floats': eng.workspace_floats(B, T, Lq, Lc), 'inference_workspace_floats': eng.inference_workspace_floats(B, T, Lq, Lc),
           'encode_workspace_floats': eng.encode_workspace_floats(B, T), 'localize_workspace_floats': eng.localize_workspace_floats(B, T, Lq, Lc)}
    out['offsets'] = {n: int(eng.lib.vsl_workspace_offset(eng.h, B, T, Lq, Lc, n.encode())) for n in OFFSET_NAMES}
    return out


def train_and_infer(cfgkw, B, T, Lq, Lc=6, lazy=True, ragged_extreme=False, bf16=False):
    import torch
    eng, flat, pad, glove, b, d = setup(cfgkw, B, T, Lq, Lc, ragged_extreme)
    if bf16:
        d['vfeats'] = d['vfeats'].to(torch.bfloat16)
    rec = {}
    eng.profile_select('*')
    h, sl, el = eng.forward(flat, pad, glove, d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], training=True, seed=STEP_SEED)
    rec.update(sizes_and_offsets(eng, B, T, Lq, Lc))
    if lazy:
        losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0, inv_batch=1.0 / B, mask_sum=float(b['v_mask'].sum()), lazy=True)
    else:
        losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    g = eng.backward(d_h, d_sl, d_el, eng.new_flat(), fused_step=dict(flat=flat, exp_avg=m, exp_avg_sq=v, lr=1e-3, step=1, clip_norm=1.0))
    si, ei = eng.extract_index(sl, el)
    torch.cuda.synchronize()
    rec['train_ledger'] = ledger(eng)
    rec['train'] = {'h_score': sha(h), 'start_logits': sha(sl), 'end_logits': sha(el), 'start_index': sha(si), 'end_index': sha(ei), 'losses': sha(losses),
                    'seeds': sha(torch.stack([d_h, d_sl, d_el])), 'grads': sha(g), 'params_after_step': sha(flat), 'exp_avg': sha(m), 'exp_avg_sq': sha(v)}
    eng.profile_select('*')
    h, sl, el = eng.forward(flat, pad, glove, d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], inference=True)
    si, ei = eng.extract_index(sl, el)
    torch.cuda.synchronize()
    rec['infer_ledger'] = ledger(eng)
    rec['infer'] = {'h_score': sha(h), 'start_logits': sha(sl), 'end_logits': sha(el), 'start_index': sha(si), 'end_index': sha(ei)}
    eng.profile_select(None)
    return rec


def shared_video(cfgkw, N, B, T, Lq, bf16, Lc=6):
    import torch
    eng, flat, pad, glove, b, d = setup(dict(cfgkw, drop_rate=0.0), B, T, Lq, Lc)
    vf = d['vfeats'][:N].contiguous()
    if bf16:
        vf = vf.to(torch.bfloat16)
    idx = [(7 * i + 3) % N for i in range(B)]          # repeated and permuted
    rec = {'encode_workspace_floats': eng.encode_workspace_floats(N, T), 'localize_workspace_floats': eng.localize_workspace_floats(B, T, Lq, Lc)}
    eng.profile_select('*')
    enc = eng.encode_video(flat, vf, d['v_mask'][:N].contiguous())
    torch.cuda.synchronize()
    rec['encode_ledger'] = ledger(eng)
    eng.profile_select('*')
    h, sl, el = eng.localize(flat, pad, glove, enc, idx, d['word_ids'], d['char_ids'], d['q_mask'])
    si, ei = eng.extract_index(sl, el)
    torch.cuda.synchronize()
    rec['localize_ledger'] = ledger(eng)
    eng.profile_select(None)
    rec['out'] = {'encoding': sha(enc.encoding), 'h_score': sha(h), 'start_logits': sha(sl), 'end_logits': sha(el), 'start_index': sha(si), 'end_index': sha(ei)}
    return rec


def shared_train(cfgkw, N, B, T, Lq, Lc=6):
    """One training step through a shared encoding: dropout on, fixed seed, lazy loss, the fused optimizer step."""
    import torch
    eng, flat, pad, glove, b, d = setup(cfgkw, B, T, Lq, Lc)
    idx = [(7 * i + 3) % N for i in range(B)]          # repeated and permuted
    vmask = d['v_mask'][:N].contiguous()
    rec = {}
    eng.profile_select('*')
    h, sl, el = eng.forward_shared(flat, pad, glove, d['word_ids'], d['char_ids'], d['vfeats'][:N].contiguous(), vmask, d['q_mask'], idx, training=True, seed=STEP_SEED)
    rec['shared_workspace_floats'] = eng.shared_workspace_floats(B, N, T, Lq, Lc)
    rec['offsets'] = {n: int(eng.lib.vsl_shared_workspace_offset(eng.h, B, N, T, Lq, Lc, n.encode())) for n in OFFSET_NAMES + SHARED_OFFSET_NAMES}
    losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0, inv_batch=1.0 / B, mask_sum=float(b['v_mask'][:N][idx].sum()), lazy=True)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    g = eng.backward(d_h, d_sl, d_el, eng.new_flat(), fused_step=dict(flat=flat, exp_avg=m, exp_avg_sq=v, lr=1e-3, step=1, clip_norm=1.0))
    si, ei = eng.extract_index(sl, el)
    torch.cuda.synchronize()
    rec['train_ledger'] = ledger(eng)
    eng.profile_select(None)
    rec['train'] = {'h_score': sha(h), 'start_logits': sha(sl), 'end_logits': sha(el), 'start_index': sha(si), 'end_index': sha(ei), 'losses': sha(losses),
                    'seeds': sha(torch.stack([d_h, d_sl, d_el])), 'grads': sha(g), 'params_after_step': sha(flat), 'exp_avg': sha(m), 'exp_avg_sq': sha(v)}
    return rec


def separate_calls(cfgkw, B, T, Lq, Lc=6):
    """The calls a fused step folds away, each on its own: the eager loss with the mask sum left to the device, the losses alone, a plain backward,
    and the optimizer step with the norm from the backward's reduction and then from its own pass over the bucket."""
    import torch
    eng, flat, pad, glove, b, d = setup(cfgkw, B, T, Lq, Lc)
    rec = {}
    eng.profile_select('*')
    h, sl, el = eng.forward(flat, pad, glove, d['word_ids'], d['char_ids'], d['vfeats'], d['v_mask'], d['q_mask'], training=True, seed=STEP_SEED)
    losses, d_h, d_sl, d_el = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0, mask_sum=0.0)
    losses_only = eng.loss(d['s_labels'], d['e_labels'], d['h_labels'], 1.0, 5.0, mask_sum=0.0, want_grads=False)[0]
    g = eng.backward(d_h, d_sl, d_el, eng.new_flat())
    m, v, gn = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(2, device='cuda')
    eng.adamw_step(flat, g, m, v, 1e-3, 1, clip_norm=1.0, grad_norm_out=gn[0:1], norm_from_backward=True)
    torch.cuda.synchronize()
    rec['step1'] = {'params': sha(flat), 'exp_avg': sha(m), 'exp_avg_sq': sha(v)}
    eng.adamw_step(flat, g, m, v, 1e-3, 2, clip_norm=1.0, grad_norm_out=gn[1:2])
    torch.cuda.synchronize()
    rec['step2'] = {'params': sha(flat), 'exp_avg': sha(m), 'exp_avg_sq': sha(v)}
    rec['calls_ledger'] = ledger(eng)
    eng.profile_select(None)
    rec['out'] = {'h_score': sha(h), 'start_logits': sha(sl), 'end_logits': sha(el), 'losses': sha(losses), 'losses_only': sha(losses_only),
                  'seeds': sha(torch.stack([d_h, d_sl, d_el])), 'grads': sha(g), 'grad_norms': sha(gn)}
    return rec


def child(out_path):
    from tests.test_dispatch_boundaries import ROWS
    cases = {}
    for p in ROWS:
        r = p.values[0]
        cases['row:' + p.id] = train_and_infer(dict(num_heads=r['heads'], predictor=r['predictor'], video_feature_dim=r['Dv'], word_dim=r['word_dim']),
                                               r['B'], r['T'], r['Lq'], lazy=r['lazy'], ragged_extreme=r['ragged'])
    for H, shapes in ((1, ATTN_SHAPES_WIDE), (2, ATTN_SHAPES_WIDE), (4, ATTN_SHAPES_LONG), (16, ATTN_SHAPES_LONG)):
        for (B, T, Lq) in shapes:
            cases['attn:H%d-B%d-T%d-Lq%d' % (H, B, T, Lq)] = train_and_infer(dict(num_heads=H, video_feature_dim=64), B, T, Lq)
    cases['headline:B64-T128-Dv1024-Lq20'] = train_and_infer(dict(video_feature_dim=1024), 64, 128, 20, Lc=10)
    cases['rnn:B96-T128-chunked'] = train_and_infer(dict(video_feature_dim=64, predictor='rnn'), 96, 128, 9)
    for pred in ('transformer', 'rnn'):
        for bf16 in (False, True):
            for (N, B, T, Lq) in ((3, 8, 64, 9), (2, 5, 160, 33)):
                cases['shared:%s-%s-N%d-B%d-T%d-Lq%d' % (pred, 'bf16' if bf16 else 'fp32', N, B, T, Lq)] = \
                    shared_video(dict(video_feature_dim=64, predictor=pred), N, B, T, Lq, bf16)
    for pred in ('transformer', 'rnn'):
        for (N, B, T, Lq) in ((3, 8, 64, 9), (2, 5, 160, 33)):
            cases['shared_train:%s-N%d-B%d-T%d-Lq%d' % (pred, N, B, T, Lq)] = shared_train(dict(video_feature_dim=64, predictor=pred), N, B, T, Lq)
    small = dict(video_feature_dim=64)
    cases['launchers:word-table-B3-T40-Lq9'] = train_and_infer(dict(small, word_table=True), 3, 40, 9)
    cases['launchers:bf16-features-B3-T40-Lq9'] = train_and_infer(small, 3, 40, 9, bf16=True)
    cases['launchers:separate-calls-B3-T40-Lq9'] = separate_calls(small, 3, 40, 9)
    cases['launchers:char100-wd52-B3-T56-Lq40'] = train_and_infer(dict(small, char_dim=100, word_dim=52), 3, 56, 40)
    cases['launchers:B3-T64-Lq100'] = train_and_infer(small, 3, 64, 100)
    with open(out_path, 'w') as f:
        json.dump(cases, f)


def dump(out_path, timeout=900):
    lib = os.environ.get('VSLNET_HIP_LIB') or os.path.join(ROOT, 'vslnet_amd', 'lib', 'libvslnet_hip.so')
    res = {'library': lib, 'library_sha256': hashlib.sha256(open(lib, 'rb').read()).hexdigest() if os.path.exists(lib) else None, 'modes': {}}
    for mode, env in MODES.items():
        part = '%s.%s.part' % (out_path, mode)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', part], env=dict(os.environ, **env), timeout=timeout)
        if r.returncode != 0:
            print('STOPPED: child of mode %s exited with status %d' % (mode, r.returncode))
            return 1
        res['modes'][mode] = json.load(open(part))
        os.remove(part)
        print('mode %s: %d cases' % (mode, len(res['modes'][mode])))
        sys.stdout.flush()
    with open(out_path, 'w') as f:
        json.dump(res, f)
    print('%s: %d cases, library %s sha256 %s' % (out_path, sum(len(m) for m in res['modes'].values()), lib, res['library_sha256']))
    return 0


def walk(a, b, path, out):
    if isinstance(a, dict) and isinstance(b, dict):
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                out.append('%s/%s: only in %s' % (path, k, 'A' if k in a else 'B'))
            else:
                walk(a[k], b[k], path + '/' + k, out)
    elif isinstance(a, list) and isinstance(b, list) and path.endswith('_ledger'):
        if len(a) != len(b):
            out.append('%s: %d launches against %d' % (path, len(a), len(b)))
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                out.append('%s[%d]: %s against %s' % (path, i, x, y))
    elif a != b:
        out.append('%s: %s against %s' % (path, a, b))


def diff(pa, pb):
    A, B = json.load(open(pa)), json.load(open(pb))
    out = []
    walk(A['modes'], B['modes'], '', out)
    for line in out:
        print(line)
    n = sum(len(m) for m in A['modes'].values())
    print('A: %s sha256 %s\nB: %s sha256 %s' % (A['library'], A['library_sha256'], B['library'], B['library_sha256']))
    print('%d cases in %d modes compared: %s' % (n, len(A['modes']), '%d DIFFERENCES' % len(out) if out else 'no difference'))
    return 1 if out else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        child(sys.argv[2])
        sys.exit(0)
    if len(sys.argv) == 3 and sys.argv[1] == 'dump':
        sys.exit(dump(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == 'diff':
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
