"""bench.py's plain line, `--full` and `--dump-outputs`: a plain run times exactly --steps steps in one region and carries none of the
--full measurements; both modes time the same steps on the same weights, so their dumped outputs agree; above the size limit the dump keeps a
fixed sample of every large array."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ['--batch', '8', '--T', '32', '--dv', '64', '--resident-batches', '2']


def test_dump_keeps_a_fixed_sample_above_the_limit(tmp_path):
    arrays = {'small': torch.arange(6, dtype=torch.float64).view(2, 3), 'big': torch.randn(1000)}
    bench.write_outputs(str(tmp_path / 'whole'), arrays)
    for k, v in arrays.items():
        got = np.load(str(tmp_path / 'whole' / (k + '.npy')))
        assert got.dtype == np.float32 and got.shape == tuple(v.shape) and np.array_equal(got, v.float().numpy())
    for run in ('a', 'b'):
        bench.write_outputs(str(tmp_path / run), arrays, limit=800)            # 100 floats per array
    a, b = np.load(str(tmp_path / 'a' / 'big.npy')), np.load(str(tmp_path / 'b' / 'big.npy'))
    assert a.shape == (100,) and np.array_equal(a, b) and np.isin(a, arrays['big'].numpy()).all()
    assert np.load(str(tmp_path / 'a' / 'small.npy')).shape == (2, 3)
    assert sum(os.path.getsize(str(tmp_path / 'a' / f)) - 128 for f in os.listdir(str(tmp_path / 'a'))) <= 800


def _run(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '2', *SHAPE, *args],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    plain = _run('--dump-outputs', str(tmp_path / 'plain'))
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in plain, k
    assert plain['steps'] == 3 and plain['regions'] == 1 and len(plain['region_ms']) == 1 and plain['ms_per_step'] > 0
    assert not {'roofline', 'cpu_baseline', 'shapes', 'allreduce_us'} & set(plain)
    full = _run('--full', '--regions', '1', '--no-cpu-baseline', '--dump-outputs', str(tmp_path / 'full'))
    assert 'roofline' in full and full['roofline']['launches_per_step'] >= 1
    p = lambda mode, k: np.load(str(tmp_path / mode / (k + '.npy')))         # noqa: E731
    shapes = {'losses': (4,), 'h_score': (8, 32), 'start_logits': (8, 32), 'end_logits': (8, 32)}
    for k in ('losses', 'h_score', 'start_logits', 'end_logits', 'grads', 'params'):
        a, b = p('plain', k), p('full', k)
        assert a.dtype == np.float32 and a.shape == b.shape == shapes.get(k, a.shape), k
        fin = np.abs(b) < 1e29                                                    # (masked logits are -1e30)
        assert np.isfinite(a).all() and np.array_equal(np.abs(a) < 1e29, fin), k
        assert float(np.abs(a - b)[fin].max()) <= 1e-4 * float(np.abs(b[fin]).max()) + 1e-6, k   # the same steps: HIP events change no result
    assert abs(float(p('plain', 'losses')[2]) - plain['config']['loss']) <= 1e-5 * abs(plain['config']['loss']) + 1e-5
    assert p('plain', 'params').shape == p('plain', 'grads').shape and p('plain', 'params').ndim == 1
