"""Golden fixtures for num_heads 1, 2, 4 and 16, produced by running the REFERENCE itself (build container only; never on the GPU box).

    python tools/make_golden_heads.py [NAME ...]        # default: every case below

Each case is oracle/make_golden.py's `tiny_tf` spec with another head count, written by its own `run_case` (oracle/ is imported, not changed).
A fixture holds about 2.4 MB of float32 data that does not compress, so it is stored as `tests/golden/<name>.npz` (config, inputs, checksums,
taps, outputs and the first gradients) plus `<name>.part<k>.npz` files with the remaining gradients, each under 1 MiB.
tests/test_attention_heads.py (load_heads_golden) merges them; tests/test_attention_heads_wide.py reads heads1_tf / heads2_tf the same way.
"""
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import CASES, load_reference, run_case  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PART_BYTES = 900 * 1024          # raw bytes per file (float32 gradients compress by a few per cent at most)
HEAD_CASES = {'heads4_tf': 4, 'heads16_tf': 16, 'heads1_tf': 1, 'heads2_tf': 2}


def split(name):
    path = os.path.join(GOLDEN, name + '.npz')
    z = dict(np.load(path, allow_pickle=False))
    for old in glob.glob(os.path.join(GOLDEN, name + '.part*.npz')):
        os.remove(old)
    grads = sorted((k for k in z if k.startswith('grad.')), key=lambda k: -z[k].nbytes)
    parts = [{k: v for k, v in z.items() if not k.startswith('grad.')}]
    sizes = [sum(v.nbytes for v in parts[0].values())]
    for k in grads:                                  # first fit, largest first
        for i, s in enumerate(sizes):
            if s + z[k].nbytes <= PART_BYTES:
                break
        else:
            parts.append({})
            sizes.append(0)
            i = len(parts) - 1
        parts[i][k] = z[k]
        sizes[i] += z[k].nbytes
    np.savez_compressed(path, **parts[0])
    for i, p in enumerate(parts[1:], 1):
        np.savez_compressed(os.path.join(GOLDEN, '%s.part%d.npz' % (name, i)), **p)
    for f in [path] + sorted(glob.glob(os.path.join(GOLDEN, name + '.part*.npz'))):
        assert os.path.getsize(f) < 1 << 20, f
        print('  %s %d KiB' % (os.path.basename(f), os.path.getsize(f) // 1024))


def main():
    VSLNet, _, _ = load_reference()
    torch.set_num_threads(8)
    names = sys.argv[1:] or list(HEAD_CASES)
    for name in names:
        heads = HEAD_CASES[name]
        over, B, T, Lq, Lc, ragged = CASES['tiny_tf']
        run_case(VSLNet, name, (dict(over, num_heads=heads), B, T, Lq, Lc, ragged))
        split(name)


if __name__ == '__main__':
    main()
