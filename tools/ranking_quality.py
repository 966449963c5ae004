"""Does the video ranking loss make the coarse stage of the corpus search find the right videos?  It records; it does not promise.

    python tools/ranking_quality.py [--out profiles/ranking_quality.txt] [--epochs 5]

Synthetic task (main.py --task synthetic --predictor transformer), same seed and epochs, three runs:
    base       --share_videos --queries_per_video 1                     (no rank loss)
    rank max   --share_videos --rank_negatives 3 --rank_relevance max
    rank mean  --share_videos --rank_negatives 3 --rank_relevance mean
Per run, on the 128 test queries against the 128 test videos: the in-video Rank@1 at IoU 0.5 and mean IoU, corpus Rank@5 at IoU 0.5 with
--corpus_prefilter 16, and from VSLNet.rank_videos (the relevance the run was trained with; max for the base run) at M = 1 / 4 / 16:
    video recall@M   the share of queries whose own video is among the M selected (chance M / 128);
    event recall@M   the share of queries for which a selected video carries the query's EVENT.  The generator gives every video one of 16 events
                     and names it in the query's first word (w_ids[0] - 2), so about 8 of the 128 test videos match a query equally well: exact-video
                     recall is capped near M / 8, event recall is not.  Chance: the mean over the queries of 1 - C(128 - c, M) / C(128, M), c = the videos of
                     the query's event.
One in sixteen in-batch negatives is a FALSE negative on this task (another video of the same event)."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MS = (1, 4, 16)


def rank_all(model, split, relevance):
    """-> (n, 16) video ranks of every record's query over the split's videos"""
    import torch
    out = []
    with torch.no_grad():
        venc = split.encode(model)
        n = len(split.records)
        d_order = torch.arange(n, device=split.device)
        for a in range(0, n, 64):
            idx = d_order[a:a + 64]
            Lq, Lc = int(split.nwords[a:a + 64].max()), int(split.nchars[a:a + 64].max())
            w, c = torch.index_select(split.d_words[:, :Lq], 0, idx), torch.index_select(split.d_chars[:, :Lq, :Lc], 0, idx)
            qenc = model.encode_query(w, c, (w != 0).float())
            out.append(model.rank_videos(venc, qenc, max(MS), relevance=relevance).video.cpu())
    return torch.cat(out).numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--epochs', type=int, default=5)
    ap.add_argument('--model_dir', default='/tmp/vsl_ranking_quality')
    a = ap.parse_args()
    import numpy as np
    import torch
    import main as cli
    from vslnet_amd import data
    from vslnet_amd.model.VSLNet import VSLNet
    from vslnet_amd import runner
    lines = []

    def emit(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
        if a.out:
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    runs = [('base', ['--queries_per_video', '1'], 'max'), ('rank max', ['--rank_negatives', '3', '--rank_relevance', 'max'], 'max'),
            ('rank mean', ['--rank_negatives', '3', '--rank_relevance', 'mean'], 'mean')]
    emit('# main.py --task synthetic --predictor transformer --share_videos, %d epochs, seed 12345; 128 test queries x 128 test videos.' % a.epochs)
    emit('# base = --queries_per_video 1 ; rank = --rank_negatives 3 --rank_lambda 1.0 --rank_temperature 0.1.  All numbers in %.')
    for name, extra, relevance in runs:
        home = os.path.join(a.model_dir, name.replace(' ', '_'))
        common = ['--task', 'synthetic', '--predictor', 'transformer', '--model_dir', home]
        quiet = lambda *x, **k: None
        cli.run(common + ['--mode', 'train', '--share_videos', '--epochs', str(a.epochs)] + extra, log=quiet)
        res = cli.run(common + ['--mode', 'test', '--corpus', '--topk', '5', '--corpus_prefilter', '16', '--corpus_relevance', relevance], log=quiet)
        # the trained model again, for the ranks themselves
        parser = cli.build_parser()
        configs = parser.parse_args(common + ['--mode', 'test'])
        dataset, feats = data.load_dataset(configs)
        configs.char_size, configs.word_size = dataset['n_chars'], dataset['n_words']
        model = VSLNet(configs=configs, word_vectors=dataset['word_vector']).cuda()
        model.load_state_dict(torch.load(runner.get_last_checkpoint(cli.model_home(configs), suffix='t7'), map_location='cuda'))
        model.eval()
        split = data.ResidentSplit(dataset['test_set'], feats, configs, 'cuda', train=False)
        ranks = rank_all(model, split, relevance)
        event = np.array([r['w_ids'][0] - 2 for r in split.records])
        video_event = np.zeros(int(split.vid_of.max()) + 1, dtype=np.int64)
        video_event[split.vid_of] = event                                   # (one record per video on this task)
        n = len(event)
        emit('%-9s in-video Rank@1 IoU 0.5 %6.2f  mIoU %6.2f | corpus Rank@5 IoU 0.5 (prefilter 16, %s) %6.2f  prefilter video recall@16 %6.2f'
             % (name, res['r1i5'], res['mIoU'], relevance, res['corpus_r_k_i5'], res['prefilter_recall_m']))
        for M in MS:
            vid = float(np.mean([split.vid_of[i] in ranks[i, :M] for i in range(n)]) * 100)
            ev = float(np.mean([event[i] in video_event[ranks[i, :M]] for i in range(n)]) * 100)
            c = np.array([(video_event == event[i]).sum() for i in range(n)])
            chance_ev = float(np.mean([1.0 - math.comb(len(video_event) - int(k), M) / math.comb(len(video_event), M) for k in c]) * 100)
            emit('%-9s M %2d  video recall %6.2f (chance %5.2f)   event recall %6.2f (chance %5.2f)' % (name, M, vid, 100.0 * M / len(video_event), ev, chance_ev))
    emit('# one in sixteen in-batch negatives is a false negative on this task: another video of the query\'s event.')
    return 0


if __name__ == '__main__':
    sys.exit(main())
