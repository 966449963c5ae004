"""main.py --mode test --window T --window_stride S: the sliding-window numbers are printed when asked for, and nothing else changes when not."""
import json
import os

import pytest


@pytest.mark.gpu
def test_cli_reports_window_numbers_only_when_asked(tmp_path):
    import main as cli
    # videos of 32 .. 64 clips, windows of 32 at stride 16: two or three windows per video
    argv = ['--task', 'synthetic', '--predictor', 'transformer', '--max_pos_len', '64', '--video_feature_dim', '64', '--batch_size', '16', '--epochs', '1',
            '--period', '100', '--synthetic_train', '64', '--synthetic_test', '32', '--model_dir', str(tmp_path), '--topk', '5']
    out = cli.run(argv + ['--mode', 'train'], log=lambda *a: None)
    cfg = json.load(open(os.path.join(out['model_dir'], 'configs.json')))
    assert cfg['window'] == 0 and cfg['window_stride'] == 0        # stored like the other flags
    plain, asked = [], []
    res = cli.run(argv + ['--mode', 'test'], log=plain.append)
    res_w = cli.run(argv + ['--mode', 'test', '--window', '32', '--window_stride', '16'], log=asked.append)
    # without the flag: the eight lines of Rank@1 + Rank@5 and their keys, nothing of the windows
    assert len(plain) == 8 and not [x for x in plain if 'indow' in x] and not [k for k in res if 'win' in k]
    # with it: the same bytes first, then four lines of Rank@1 / mean IoU and four of Rank@5
    assert asked[:8] == plain and len(asked) == 16 and {k: v for k, v in res_w.items() if k in res} == res
    assert asked[8].startswith('\x1b[1;31mWindows 32/16 Rank@1, IoU=0.3:\t') and asked[11].startswith('\x1b[1;31mWindows 32/16 mean IoU:\t')
    assert asked[12].startswith('\x1b[1;31mWindows 32/16 Rank@5, IoU=0.3:\t') and asked[15].startswith('\x1b[1;31mWindows 32/16 best-of-5 mean IoU:\t')
    assert (res_w['window'], res_w['window_stride']) == (32, 16)
    assert 0.0 <= res_w['win_r1i7'] <= res_w['win_r1i5'] <= res_w['win_r1i3'] <= 100.0 and 0.0 <= res_w['win_mIoU'] <= res_w['win_mIoU_k'] <= 100.0
    assert res_w['win_r1i5'] <= res_w['win_r_k_i5'] <= 100.0
    # without --topk: the four Rank@1 lines alone
    only = []
    cli.run(argv + ['--mode', 'test', '--topk', '0', '--window', '32', '--window_stride', '16'], log=only.append)
    assert len(only) == 8 and only[4].startswith('\x1b[1;31mWindows 32/16 Rank@1, IoU=0.3:\t') and not [x for x in only if 'Rank@5' in x]
