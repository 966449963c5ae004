"""Two-stage corpus search, the written specification (CPU): vslnet_amd.spans.pair_relevance_reference and select_topm_reference -- what
tests/test_video_ranking.py compares the device with -- checked against definitions that share no code with them, and the public surface: the
header's declarations, the ctypes mirrors, the Engine / VSLNet methods and arguments."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests.helpers import ROOT
from vslnet_amd.spans import pair_relevance_reference, select_topm_reference


def _brute_force_topm(key, M):
    """rank of element i = the number of elements strictly in front of it: a larger key (-0.0 == +0.0), or an equal key at a smaller index.  O(N^2)."""
    G, N = key.shape
    n = min(M, N)
    index, out_key = np.full((G, M), -1, np.int32), np.zeros((G, M), np.float32)
    for g in range(G):
        for i in range(N):
            rank = sum(1 for j in range(N) if key[g, j] > key[g, i] or (key[g, j] == key[g, i] and j < i))
            if rank < n:
                index[g, rank], out_key[g, rank] = i, key[g, i]
    return index, out_key, np.full(G, n, np.int32)


@pytest.mark.parametrize('seed', range(6))
def test_select_topm_reference_equals_a_rank_count(seed):
    rng = np.random.default_rng(seed)
    values = np.array([[-np.inf, -0.0, 0.0, 1.5], [-2.0, -0.0, 0.0, np.inf], [0.25, 0.5, -0.0, 0.0]][seed % 3], np.float32)
    for N in (1, 2, 7, 33):
        key = values[rng.integers(0, 4, size=(3, N))]                       # four distinct values (two of them the two zeros): ties dominate
        for M in (1, 2, N - 1, N, N + 3):
            if M < 1:
                continue
            got, want = select_topm_reference(key, M), _brute_force_topm(key, M)
            assert np.array_equal(got[0], want[0]), (N, M, key, got[0], want[0])
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int32
            assert not np.signbit(got[1][got[1] == 0]).any()                # a zero comes back as +0.0


def test_select_topm_reference_orders_zeros_by_index_and_fills_the_tail():
    key = np.array([[0.0, -0.0, -np.inf, -0.0, 3.0]], np.float32)
    index, out_key, count = select_topm_reference(key, 7)
    assert index.tolist() == [[4, 0, 1, 3, 2, -1, -1]] and count.tolist() == [5]
    assert out_key.tolist() == [[3.0, 0.0, 0.0, 0.0, -np.inf, 0.0, 0.0]] and not np.signbit(out_key[0, 1:4]).any()


def test_pair_relevance_reference_on_hand_made_rows():
    h = np.array([[0.1, 0.9, 0.3, 0.7], [0.5, 0.2, 0.8, 0.6], [0.4, 0.4, 0.4, 0.4], [0.3, 0.1, 0.2, 0.0]], np.float32)
    mask = np.array([[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 1]], np.float32)      # row 2: all pad; row 3: a mask that is no prefix
    mx, mean = pair_relevance_reference(h, mask, 'max'), pair_relevance_reference(h, mask, 'mean')
    assert mx.dtype == np.float32 and mx.tolist() == [np.float32(0.9), np.float32(0.5), -np.inf, np.float32(0.1)]
    rows = [[float(x) for x in h[0]], [float(h[1, 0]), float(h[1, 1])], [float(h[3, 1]), float(h[3, 3])]]      # (a float32 is exact as a Python float)
    want = [np.float32(math.fsum(r) / len(r)) for r in rows]
    assert [mean[0], mean[1], mean[3]] == want and mean[2] == -np.inf and mean.dtype == np.float32
    lengths = np.array([4, 2, 0, 1])
    assert pair_relevance_reference(h, lengths, 'max').tolist() == [np.float32(0.9), np.float32(0.5), -np.inf, np.float32(0.3)]
    with pytest.raises(ValueError, match="'max' or 'mean'"):
        pair_relevance_reference(h, mask, 'sum')


def _header():
    return open(os.path.join(ROOT, 'include', 'vslnet_hip.h')).read()


def test_header_declares_the_entry_points_and_the_mirrors_match():
    from vslnet_amd import build, engine
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    assert re.search(r'int vsl_highlight_pairs\(vsl_handle h, const vsl_highlight_io\* io, void\* hip_stream\);', src)
    assert re.search(r'int vsl_select_topm\(vsl_handle h, const vsl_select_io\* io, void\* hip_stream\);', src)
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', src)                 # an added entry point does not move the version
    lib = ctypes.CDLL(build.build())
    for s in ('vsl_highlight_pairs', 'vsl_select_topm'):
        assert hasattr(lib, s) and s in engine.ABI_SYMBOLS, s
    assert 'kernels_rank.hip' in build.SOURCES
    # (the mirrors of vsl_pairs_io, vsl_highlight_io and vsl_select_io against the header and the host compiler: tests/test_abi_layout.py, as for
    # every struct)
    assert engine.TOPM_MAX_M == 1024 and re.search(r'constexpr int TOPM_MAX_M = 1024;', open(os.path.join(ROOT, 'vslnet_amd', 'csrc', 'launch.hpp')).read())


def test_engine_and_module_expose_the_new_calls():
    from vslnet_amd.engine import Engine, VideoRanks
    from vslnet_amd.model.VSLNet import VSLNet
    assert VideoRanks._fields == ('video', 'relevance', 'count')
    sig = inspect.signature(Engine.highlight_pairs).parameters
    assert list(sig)[1:] == ['flat', 'venc', 'qenc', 'video_index', 'query_index', 'relevance', 'out', 'ld', 'h_score']
    assert (sig['relevance'].default, sig['out'].default, sig['ld'].default, sig['h_score'].default) == ('max', None, 0, None)
    assert list(inspect.signature(Engine.select_topm).parameters)[1:] == ['key', 'M']
    sig = inspect.signature(VSLNet.rank_videos).parameters
    assert list(sig)[1:] == ['venc', 'qenc', 'm', 'relevance', 'pairs_per_call'] and (sig['relevance'].default, sig['pairs_per_call'].default) == ('max', 4096)
    sig = inspect.signature(VSLNet.retrieve).parameters
    assert list(sig)[1:10] == ['venc', 'qenc', 'k', 'nms_iou', 'max_span', 'lengths', 'pairs_per_call', 'prefilter', 'relevance']
    assert (sig['prefilter'].default, sig['relevance'].default, sig['pairs_per_call'].default, sig['nms_iou'].default) == (0, 'max', 4096, 0.5)


def test_runner_and_cli_defaults():
    import argparse
    import json
    import main as cli
    from vslnet_amd import runner
    sig = inspect.signature(runner.eval_corpus).parameters
    assert (sig['prefilter'].default, sig['relevance'].default) == (0, 'max')
    ns = cli.build_parser().parse_args([])
    assert (ns.corpus_prefilter, ns.corpus_relevance) == (0, 'max') and cli.prefilter_of(ns) == (0, 'max')
    # a configs.json from before the flags reads back as the defaults
    stored = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'ref_checkpoint', 'configs.json')))
    assert 'corpus_prefilter' not in stored and 'corpus_relevance' not in stored
    p = cli.build_parser()
    p.set_defaults(**stored)
    assert cli.prefilter_of(p.parse_args([])) == (0, 'max')
    assert cli.prefilter_of(argparse.Namespace(**stored)) == (0, 'max')
