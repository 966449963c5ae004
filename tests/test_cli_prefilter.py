"""main.py --corpus_prefilter / --corpus_relevance: the coarse-to-fine corpus search from the command line (runner.eval_corpus(prefilter=M))."""
import json
import os

import pytest


def test_prefilter_flags_belong_to_corpus():
    """argparse only (CPU): both flags are refused without --corpus, with a message; with it they parse"""
    import main as cli
    p = cli.build_parser()
    for argv in (['--corpus_prefilter', '4'], ['--mode', 'test', '--topk', '3', '--corpus_prefilter', '4'], ['--corpus_relevance', 'mean']):
        with pytest.raises(ValueError, match='--corpus_prefilter / --corpus_relevance need --corpus'):
            cli.prefilter_of(p.parse_args(argv))
    with pytest.raises(ValueError, match='--corpus_prefilter -2: at least 0'):
        cli.prefilter_of(p.parse_args(['--corpus', '--corpus_prefilter', '-2']))
    with pytest.raises(SystemExit):
        p.parse_args(['--corpus', '--corpus_relevance', 'sum'])
    assert cli.prefilter_of(p.parse_args(['--mode', 'test', '--corpus', '--topk', '3', '--corpus_prefilter', '4', '--corpus_relevance', 'mean'])) == (4, 'mean')
    assert cli.prefilter_of(p.parse_args(['--corpus'])) == (0, 'max')
    # run() refuses before it builds anything
    with pytest.raises(ValueError, match='need --corpus'):
        cli.run(['--task', 'synthetic', '--mode', 'test', '--topk', '3', '--corpus_prefilter', '4'], log=lambda *a: None)


@pytest.mark.gpu
def test_cli_reports_the_prefilter_recall_only_when_asked(tmp_path):
    import main as cli
    argv = ['--task', 'synthetic', '--predictor', 'transformer', '--max_pos_len', '32', '--video_feature_dim', '64', '--batch_size', '16', '--epochs', '1',
            '--period', '100', '--synthetic_train', '64', '--synthetic_test', '32', '--model_dir', str(tmp_path), '--topk', '3']
    out = cli.run(argv + ['--mode', 'train'], log=lambda *a: None)
    stored = json.load(open(os.path.join(out['model_dir'], 'configs.json')))
    assert stored['corpus_prefilter'] == 0 and stored['corpus_relevance'] == 'max'              # stored like the other flags
    plain, coarse, every = [], [], []
    res = cli.run(argv + ['--mode', 'test', '--corpus'], log=plain.append)
    res_c = cli.run(argv + ['--mode', 'test', '--corpus', '--corpus_prefilter', '4'], log=coarse.append)
    # without the flag: the eight lines of Rank@1 + Rank@3 and the three corpus lines, as before; no prefilter key
    assert len(plain) == 11 and not [x for x in plain if 'refilter' in x] and not [k for k in res if 'prefilter' in k]
    # with it: the same bytes first, then the prefilter recall line, then the three corpus lines
    assert coarse[:8] == plain[:8] and len(coarse) == 12
    assert coarse[8].startswith('\x1b[1;31mPrefilter (max) video recall@4:\t') and coarse[9].startswith('\x1b[1;31mCorpus Rank@3, IoU=0.5:\t')
    assert coarse[11].startswith('\x1b[1;31mvideo Recall@3:\t')
    assert res_c['prefilter_m'] == 4 and {k: v for k, v in res_c.items() if k in res and 'corpus' not in k and 'recall' not in k} == \
        {k: v for k, v in res.items() if 'corpus' not in k and 'recall' not in k}
    # a moment can only be returned from a selected video
    assert 0.0 <= res_c['corpus_r_k_i7'] <= res_c['corpus_r_k_i5'] <= res_c['video_recall_k'] <= res_c['prefilter_recall_m'] <= 100.0
    # every video kept (more than 1024 asked of a split of at most 32 videos): the exhaustive numbers, and every ground-truth video is among the selected
    res_a = cli.run(argv + ['--mode', 'test', '--corpus', '--corpus_prefilter', '2000', '--corpus_relevance', 'mean'], log=every.append)
    assert every[8].startswith('\x1b[1;31mPrefilter (mean) video recall@2000:\t100.00') and every[9:] == plain[8:]
    assert res_a['prefilter_recall_m'] == 100.0 and {k: res_a[k] for k in res} == res
