"""Sliding windows over a video of any length, the CPU half: the written specification of the cross-window merge (vslnet_amd.spans.merge_windows_reference)
against hand-worked cases, the window table (vslnet_amd.spans.window_table) and the exports of the built library.  The GPU half is tests/test_windows.py."""
import ctypes

import numpy as np
import pytest

from vslnet_amd.spans import merge_topk_reference, merge_windows_reference, window_table

NEW_SYMBOLS = ('vsl_encode_windows', 'vsl_encode_windows_workspace_floats', 'vsl_merge_windows')
F32, I32, I64 = np.float32, np.int32, np.int64


def _lists(start, end, key, score=None):
    start, end, key = np.asarray(start, dtype=I64), np.asarray(end, dtype=I64), np.asarray(key, dtype=F32)
    score = np.asarray(score, dtype=F32) if score is not None else (10.0 * key).astype(F32)
    return start, end, score, key


# ------------------------------------------------------------------------------------------------ the specification
def test_a_duplicate_from_two_windows_appears_once_and_offsets_shift_the_spans():
    # window 0 starts at clip 0, window 1 at clip 16: local (20, 25) of window 0 and local (4, 9) of window 1 are the same moment
    start, end, score, key = _lists([[20, 2], [4, 10]], [[25, 3], [9, 12]], [[0.9, 0.3], [0.8, 0.5]])
    count, group, offset = np.array([2, 2], I32), np.array([0, 0], I32), np.array([0, 16], I32)
    lst, s, e, sc, k, c = merge_windows_reference(start, end, score, key, count, group, 1, 5, 1.0, offset)
    assert c.tolist() == [3]                                     # four candidates, one of them a duplicate: nms_iou = 1 removes duplicates only
    assert s[0, :3].tolist() == [20, 26, 2] and e[0, :3].tolist() == [25, 28, 3] and lst[0, :3].tolist() == [0, 1, 0]
    assert np.array_equal(k[0, :3], np.array([0.9, 0.5, 0.3], F32)) and np.array_equal(sc[0, :3], np.array([9.0, 5.0, 3.0], F32))
    assert (lst[0, 3:] == -1).all() and (s[0, 3:] == -1).all() and (e[0, 3:] == -1).all() and np.isneginf(sc[0, 3:]).all() and (k[0, 3:] == 0).all()
    assert (lst.dtype, s.dtype, e.dtype, sc.dtype, k.dtype, c.dtype) == (I32, I64, I64, F32, F32, I32)
    # the duplicate with the larger key wins whichever window it is in
    start, end, score, key = _lists([[20], [4]], [[25], [9]], [[0.4], [0.8]])
    lst, s, e, _, k, c = merge_windows_reference(start, end, score, key, np.array([1, 1], I32), group, 1, 2, 1.0, offset)
    assert c.tolist() == [1] and lst[0, 0] == 1 and (s[0, 0], e[0, 0]) == (20, 25) and k[0, 0] == F32(0.8)
    # without offsets the two are different spans
    c = merge_windows_reference(start, end, score, key, np.array([1, 1], I32), group, 1, 2, 1.0)[5]
    assert c.tolist() == [2]


def test_nms_across_windows_and_disjoint_spans_at_zero():
    # global spans: A (0, 9) key .9 | B (5, 14) key .8 (iou with A 5 / 15) | C (10, 19) key .7 (disjoint from A, iou with B 5 / 15) | D (9, 9) key .6 (inside A)
    start, end, score, key = _lists([[0, 5], [2, 1]], [[9, 14], [11, 1]], [[0.9, 0.8], [0.7, 0.6]])
    count, group, offset = np.array([2, 2], I32), np.array([0, 0], I32), np.array([0, 8], I32)
    at = lambda iou: merge_windows_reference(start, end, score, key, count, group, 1, 4, iou, offset)      # noqa: E731
    lst, s, e, _, _, c = at(0.0)                                 # mutually disjoint spans only
    assert c.tolist() == [2] and s[0, :2].tolist() == [0, 10] and e[0, :2].tolist() == [9, 19]
    lst, s, e, _, _, c = at(0.3)                                 # B (1 / 3 > 0.3) and D (1 / 10 <= 0.3 stays) ; C stays
    assert c.tolist() == [3] and s[0, :3].tolist() == [0, 10, 9]
    lst, s, e, _, _, c = at(0.5)
    assert c.tolist() == [4] and s[0, :4].tolist() == [0, 5, 10, 9]
    assert at(1.0)[5].tolist() == [4]


def test_ties_break_by_global_start_then_end_then_list_then_slot():
    key = np.full((3, 2), 0.5, F32)
    #           list 0: (12, 20), (12, 15)      list 1 (+10): (1, 3) -> (11, 13), (2, 5) -> (12, 15) a duplicate of list 0's      list 2: (12, 20) a duplicate too
    start, end = np.array([[12, 12], [1, 2], [12, 3]], I64), np.array([[20, 15], [3, 5], [20, 3]], I64)
    score = np.arange(6, dtype=F32).reshape(3, 2)
    count, group, offset = np.array([2, 2, 2], I32), np.zeros(3, I32), np.array([0, 10, 0], I32)
    lst, s, e, sc, _, c = merge_windows_reference(start, end, score, key, count, group, 1, 8, 1.0, offset)
    assert c.tolist() == [4]
    assert list(zip(s[0, :4].tolist(), e[0, :4].tolist())) == [(3, 3), (11, 13), (12, 15), (12, 20)]
    assert lst[0, :4].tolist() == [2, 1, 0, 0]                   # (12, 15): list 0 before list 1 ; (12, 20): list 0 before list 2
    assert sc[0, :4].tolist() == [5.0, 2.0, 1.0, 0.0]
    # the same list holds one span twice: the smaller slot wins
    start, end = np.array([[4, 4]], I64), np.array([[6, 6]], I64)
    lst, s, e, sc, _, c = merge_windows_reference(start, end, np.array([[1.0, 2.0]], F32), np.full((1, 2), 0.5, F32), np.array([2], I32), np.zeros(1, I32), 1, 2, 0.5)
    assert c.tolist() == [1] and sc[0, 0] == 1.0


def test_empty_lists_and_lists_in_no_group():
    start, end, score, key = _lists([[1, 2], [3, 4], [5, 6], [7, 8]], [[1, 2], [3, 4], [5, 6], [7, 8]], [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6], [0.7, 0.8]])
    count = np.array([0, 2, 2, 5], I32)                          # list 0 is empty ; list 3's count exceeds K: clamped
    group = np.array([0, -1, 3, 2], I32)                         # list 1 and list 2 (G = 3) are in no group
    lst, s, e, sc, k, c = merge_windows_reference(start, end, score, key, count, group, 3, 3, 0.5)
    assert c.tolist() == [0, 0, 2] and s[2, :2].tolist() == [8, 7] and (lst[:2] == -1).all() and (k[:2] == 0).all()
    c = merge_windows_reference(start, end, score, key, count, np.array([2 ** 31 - 1, -2 ** 31, 7, 9], I32), 3, 3, 0.5)[5]
    assert c.tolist() == [0, 0, 0]


def test_without_offsets_duplicates_and_nms_it_is_the_plain_merge():
    rng = np.random.default_rng(41)
    B, K, G = 40, 4, 3
    key = rng.permutation(B * K).reshape(B, K).astype(F32) / F32(B * K)       # distinct keys
    start = np.arange(B * K, dtype=I64).reshape(B, K) * 3                       # no two spans identical
    end = start + rng.integers(0, 40, (B, K))
    score = rng.standard_normal((B, K)).astype(F32)
    count, group = rng.integers(0, K + 1, B).astype(I32), rng.integers(-1, G + 1, B).astype(I32)
    lst, s, e, sc, k, c = merge_windows_reference(start, end, score, key, count, group, G, 7, 1.0, np.zeros(B, I32))
    ref = merge_topk_reference(start, end, score, key, count, group, G, 7, tag=np.zeros(B, I32))
    assert np.array_equal(lst, ref[1]) and np.array_equal(s, ref[2]) and np.array_equal(e, ref[3])
    assert np.array_equal(sc.view(I32), ref[4].view(I32)) and np.array_equal(k.view(I32), ref[5].view(I32)) and np.array_equal(c, ref[6])
    assert (c > 0).any()


# ------------------------------------------------------------------------------------------------ the window table
@pytest.mark.parametrize('window,stride', [(32, 16), (24, 24), (37, 5)])
@pytest.mark.parametrize('L', [10, 24, 32, 33, 75])
def test_window_table_covers_every_clip(L, window, stride):
    start, length = window_table(L, window, stride)
    W = 1 if L <= window else -(-(L - window) // stride) + 1
    assert len(start) == len(length) == W and start.tolist() == [w * stride for w in range(W)]
    covered = np.zeros(L, dtype=bool)
    for s, n in zip(start, length):
        assert 1 <= n <= window and s + n <= L
        covered[s:s + n] = True
    assert covered.all()
    assert length[-1] == min(window, L - (W - 1) * stride) and start[-1] + length[-1] == L
    assert (length[:-1] == window).all()                        # only the last window may be short
    if W > 1:
        assert start[-2] + window < L                           # ... and it is needed: the one before it does not reach the end


def test_window_table_hand_cases_and_refusals():
    assert [x.tolist() for x in window_table(75, 32, 16)] == [[0, 16, 32, 48], [32, 32, 32, 27]]
    assert [x.tolist() for x in window_table(33, 32, 16)] == [[0, 16], [32, 17]]
    assert [x.tolist() for x in window_table(10, 32, 16)] == [[0], [10]]
    assert [x.tolist() for x in window_table(48, 24, 24)] == [[0, 24], [24, 24]]
    with pytest.raises(ValueError, match='skip clips'):
        window_table(75, 16, 17)
    with pytest.raises(ValueError, match='at least 1'):
        window_table(75, 16, 0)


# ------------------------------------------------------------------------------------------------ the ABI
def test_library_exports_the_window_entry_points():
    from vslnet_amd import build, engine
    lib = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in engine.ABI_SYMBOLS, s
    assert lib.vsl_abi_version() == 9 == engine.ABI_VERSION       # an added entry point does not change the version
    # (the mirrors of vsl_encode_windows_io and vsl_merge_windows_io against the header: tests/test_abi_layout.py, as for every struct)


def test_cli_flags_are_off_by_default_and_checked():
    import main as cli
    ns = cli.build_parser().parse_args([])
    assert ns.window == 0 and ns.window_stride == 0 and cli.window_of(ns) is None
    assert cli.window_of(cli.build_parser().parse_args(['--window', '32'])) is None                         # (--mode train only stores the flags)
    assert cli.window_of(cli.build_parser().parse_args(['--mode', 'test', '--window', '32'])) == (32, 16)
    assert cli.window_of(cli.build_parser().parse_args(['--mode', 'test', '--window', '32', '--window_stride', '8'])) == (32, 8)
    with pytest.raises(ValueError, match='--data resident'):
        cli.window_of(cli.build_parser().parse_args(['--mode', 'test', '--window', '32', '--data', 'loader']))
    with pytest.raises(ValueError, match='--max_pos_len'):
        cli.window_of(cli.build_parser().parse_args(['--mode', 'test', '--window', '129']))
    with pytest.raises(ValueError, match='skip clips'):
        cli.window_of(cli.build_parser().parse_args(['--mode', 'test', '--window', '32', '--window_stride', '33']))
