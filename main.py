"""Command line of the MI355X-native VSLNet path: same flags and behaviour as the reference's `main_t7.py` (flags :13-45,
training loop :83-129, test mode :131-149; the TF spelling `--hidden_size` of main.py:27 is accepted for `--dim`).

    python main.py --task charades --predictor transformer --mode train          # needs the reference's processed dataset
    python main.py --task synthetic --predictor transformer --mode train --epochs 5
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py --task synthetic ...   # data parallel

What differs from the reference, by design:
  * the model is `vslnet_amd.model.VSLNet` (hand-written gfx950 kernels behind the reference's module API);
  * `--optimizer fused` (default) runs forward / losses / backward through the engine and the update as the library's fused
    clip + AdamW step on the flat parameter bucket; `--optimizer torch` is the reference's loop verbatim in structure
    (module API, `clip_grad_norm_`, `torch.optim.AdamW`, LambdaLR) -- single process only;
  * under torch.distributed.run every rank draws the same shuffled global batch and keeps its contiguous slice; losses are
    normalised with the GLOBAL batch size / mask sum, the dropout counters continue at the shard's first sample (so the
    masks, hence the training trajectory, do not depend on the number of ranks), gradients are summed with one all-reduce
    of the flat bucket
    (vslnet_amd/dp.py), the update is identical on every rank; rank 0 evaluates and writes checkpoints;
  * `--data resident` (default): each split is uploaded to HBM once (vslnet_amd/data.py: ResidentSplit) and a batch is a
    device gather with the shapes / contents of the reference's collate functions; `--data loader` keeps the reference's
    host-side collate + per-step H2D copy (measured: 39 ms/step end to end against a 1.2 ms model step);
  * `--accum_steps K`: one optimizer step over K micro-batches (gradient accumulation).  `--batch_size` stays the GLOBAL batch and the number of
    steps, the schedule, the seeds and the evaluation cadence do not change; each batch runs as K contiguous pieces, every piece a data-parallel
    shard run in sequence (global widths and normalisers, dropout counters continued at its first row), the library's backward adding to the flat
    bucket and the last piece applying clip + AdamW to the sum.  A global batch whose workspace does not fit runs as pieces that do.  Single
    process, `--optimizer fused`, not with `--share_videos`;
  * `--topk K` (with `--nms_iou`, `--max_span`): every evaluation -- `--mode test` and the ones inside training, with and without `--share_videos` --
    also asks the library for the K best moments per query (greedy temporal NMS, vsl_extract_topk) and reports Rank@K at IoU 0.3 / 0.5 / 0.7 and the
    best-of-K mean IoU beside the Rank@1 numbers, which stay those of extract_index.  0 (default): off, the output is what it was.  Like the other
    flags they go into configs.json and come back as defaults in --mode test (trained with --topk 5: Rank@5 there unless --topk 0 is given);
  * `--corpus` (`--mode test`, `--data resident`, `--topk K` >= 1): after the usual numbers, every query of the test split is also run against EVERY
    video of the split (runner.eval_corpus: videos and queries encoded once, VSLNet.retrieve ranks the moments of all videos on the device) and
    corpus Rank@K at IoU 0.5 / 0.7 -- a returned moment in the ground-truth video at that IoU -- and video Recall@K are reported.  Off by default:
    nothing printed or written changes.  `--mode train` only stores the flag in configs.json, where --mode test finds it as its default;
  * `--corpus_prefilter M` (with `--corpus_relevance max|mean`; only with `--corpus`): the corpus search runs coarse to fine -- every query's videos are
    ranked by the highlight score first (VSLNet.rank_videos) and the query is localised in its M best videos only -- and prefilter video recall@M, the
    share of queries whose ground-truth video is among the M selected, is reported in front of the corpus numbers.  0 (default): every video,
    nothing printed changes.  Stored in configs.json like the other flags;
  * `--window T --window_stride S` (`--mode test`, `--data resident`): after the usual numbers, every record of the test split is also evaluated by
    sliding windows of T clips at stride S over the clip sequence the split holds (runner.eval_windows: VSLNet.encode_windows + localize_long, the
    windows' moments merged on the device into the video's own clips) and Rank@1 / mean IoU of the first merged moment -- with `--topk K` also Rank@K
    over the K merged moments -- are reported.  0 (default): off, nothing printed or written changes.  `--mode train` only stores the flags in
    configs.json, where --mode test finds them as its defaults;
  * `--rank_negatives n` (with `--rank_lambda`, `--rank_temperature`, `--rank_relevance max|mean`; `--mode train --share_videos`, `--data resident`,
    `--optimizer fused`, `--accum_steps 1`): the video ranking loss.  `--batch_size` stays the number of pair ROWS of a step; a step takes
    batch_size // (1 + n) queries, pairs each with its own video and with up to n other videos of the step (ResidentSplit.shards(negatives=n)) and
    adds rank_lambda times a softmax ranking term over every query's video relevances -- the max / mean of the highlight score that
    `--corpus_prefilter` ranks by -- to the loss (Engine.group_loss).  The log line then also shows the rank term and hits / groups.  0 (default):
    nothing that is enqueued, printed or written changes.  --mode test takes the stored --rank_relevance as its default --corpus_relevance;
  * `--task synthetic` builds a small learnable dataset in the reference's record format (no dataset files needed).
"""
import argparse
import json
import os
import time

# RCCL brings its own streams; with ROCm's default of 4 hardware queues per process the library's two side streams then share
# a queue with another stream and the fork/join overlap of the step is lost (measured: 1.25 -> 1.51 ms/step as soon as the
# process group exists).  Must be set before the HIP runtime initialises.
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import sys

import torch

from vslnet_amd import data, dp, runner


def build_parser():
    p = argparse.ArgumentParser()
    # data parameters (main_t7.py:14-18)
    p.add_argument('--save_dir', type=str, default='datasets_t7', help='path to save processed dataset')
    p.add_argument('--task', type=str, default='charades', help='[charades | activitynet | tacos | synthetic]')
    p.add_argument('--fv', type=str, default='new', help='[new | org] for visual features')
    p.add_argument('--max_pos_len', type=int, default=128, help='maximal position sequence length allowed')
    # model parameters (:20-29)
    p.add_argument('--word_size', type=int, default=None)
    p.add_argument('--char_size', type=int, default=None)
    p.add_argument('--word_dim', type=int, default=300)
    p.add_argument('--video_feature_dim', type=int, default=1024)
    p.add_argument('--char_dim', type=int, default=50)
    p.add_argument('--dim', '--hidden_size', dest='dim', type=int, default=128, help='hidden size')
    p.add_argument('--highlight_lambda', type=float, default=5.0)
    p.add_argument('--num_heads', type=int, default=8)
    p.add_argument('--drop_rate', type=float, default=0.2)
    p.add_argument('--predictor', type=str, default='rnn', help='[rnn | transformer]')
    # training / evaluation parameters (:31-45)
    p.add_argument('--gpu_idx', type=str, default='0')
    p.add_argument('--seed', type=int, default=12345)
    p.add_argument('--mode', type=str, default='train', help='[train | test]')
    p.add_argument('--epochs', type=int, default=100)
    p.add_argument('--batch_size', type=int, default=16, help='GLOBAL batch size (split over the ranks under torchrun)')
    p.add_argument('--num_train_steps', type=int, default=None)
    p.add_argument('--init_lr', type=float, default=0.0001)
    p.add_argument('--clip_norm', type=float, default=1.0)
    p.add_argument('--warmup_proportion', type=float, default=0.0)
    p.add_argument('--extend', type=float, default=0.1, help='accepted and ignored: the reference collate hard-codes 0.1 (data_loader_t7.py:42)')
    p.add_argument('--adamw', default='torch', choices=('torch', 'hf'), help="update ordering of the fused optimizer: torch.optim.AdamW, or the historical transformers.AdamW the reference imports")
    p.add_argument('--period', type=int, default=100)
    p.add_argument('--model_dir', type=str, default='ckpt_t7')
    p.add_argument('--model_name', type=str, default='vslnet')
    p.add_argument('--suffix', type=str, default=None)
    # additions of this build
    p.add_argument('--optimizer', type=str, default='fused', help='[fused | torch]')
    p.add_argument('--data', type=str, default='resident', help='[resident | loader] resident: the whole split lives in HBM and a '
                   'batch is a device gather; loader: host-side collate + H2D copy per step, like the reference')
    p.add_argument('--share_videos', action='store_true', help='--mode test with --data resident: encode every video once and localise each '
                   'query against the resident encoding (runner.eval_test_shared); every batch is then padded to the split\'s longest video.  '
                   '--mode train with --data resident, one process: batches grouped by video (--queries_per_video) and the training step through a '
                   'shared encoding (Engine.forward_shared): the video half runs once per video, forward and backward')
    p.add_argument('--queries_per_video', type=int, default=4, help='--mode train --share_videos: queries of one video per group of the grouped order')
    p.add_argument('--accum_steps', type=int, default=1, help='gradient accumulation: every global batch of --batch_size runs as this many contiguous '
                   'micro-batches and ONE optimizer step (1: off).  Single process, --optimizer fused, not with --share_videos')
    p.add_argument('--topk', type=int, default=0, help='evaluations also report Rank@K over the K best moments per query (1..32; 0: off)')
    p.add_argument('--nms_iou', type=float, default=0.5, help='--topk: a candidate whose temporal IoU with an already chosen moment exceeds this is suppressed '
                   '(1.0: plain top-K, 0.0: disjoint moments only)')
    p.add_argument('--max_span', type=int, default=0, help='--topk: longest candidate moment in clips (0: unlimited)')
    p.add_argument('--corpus', action='store_true', help='--mode test with --data resident and --topk K >= 1: also run every query against EVERY video of '
                   'the test split (runner.eval_corpus) and report corpus Rank@K at IoU 0.5 / 0.7 and video Recall@K')
    p.add_argument('--corpus_prefilter', type=int, default=0, help='--corpus: coarse to fine -- rank the videos of the split by highlight score first and '
                   'localise each query only in its M best videos (VSLNet.retrieve prefilter=M); also reports prefilter video recall@M.  0: every video')
    p.add_argument('--corpus_relevance', choices=('max', 'mean'), default='max', help='--corpus_prefilter: a video\'s relevance to a query is the max or '
                   'the mean of the highlight score over its clips')
    p.add_argument('--rank_negatives', type=int, default=0, help='--mode train --share_videos: the video ranking loss -- every query is also paired with up '
                   'to this many other videos of its step and a softmax ranking term over the videos\' relevances is added to the loss (0: off)')
    p.add_argument('--rank_lambda', type=float, default=None, help='--rank_negatives: weight of the ranking term (1.0)')
    p.add_argument('--rank_temperature', type=float, default=None, help='--rank_negatives: temperature of the softmax over the relevances (0.1)')
    p.add_argument('--rank_relevance', choices=('max', 'mean'), default=None, help='--rank_negatives: the relevance of a video is the max or the mean of '
                   'the highlight score over its clips (max); --mode test takes it as the default of --corpus_relevance')
    p.add_argument('--window', type=int, default=0, help='--mode test with --data resident: also evaluate every record by sliding windows of this many clips '
                   '(runner.eval_windows; at most --max_pos_len; 0: off)')
    p.add_argument('--window_stride', type=int, default=0, help='--window: clips between two window starts (1 .. --window; 0: half the window)')
    p.add_argument('--synthetic_train', type=int, default=512)
    p.add_argument('--synthetic_test', type=int, default=128)
    return p


def model_home(configs):
    """main_t7.py:70-74."""
    home = os.path.join(configs.model_dir, '_'.join([configs.model_name, configs.task, configs.fv, str(configs.max_pos_len), configs.predictor]))
    if configs.suffix is not None:
        home = home + '_' + configs.suffix
    return os.path.join(home, 'model')


def _dist_env():
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (('WORLD_SIZE', '1'), ('RANK', '0'), ('LOCAL_RANK', '0')))
    return world, rank, local


def _to_device(batch, device):
    return [t.to(device, non_blocking=True) if torch.is_tensor(t) else t for t in batch]


def check_accum(configs, world):
    """--accum_steps and what it does not combine with.  -> K"""
    accum = getattr(configs, 'accum_steps', None)
    accum = 1 if accum is None else int(accum)          # (a configs.json from before the flag has none)
    if accum < 1:
        raise ValueError('--accum_steps %d: at least 1' % accum)
    if accum > 1 and configs.mode.lower() == 'train':
        if configs.optimizer != 'fused':
            raise ValueError('--accum_steps > 1 with --optimizer torch is refused: autograd already accumulates into .grad there; '
                             'the accumulated step is the production path (--optimizer fused)')
        if world > 1:
            raise ValueError('--accum_steps > 1 is single-process (world = %d): data parallel x accumulation needs the gradient exchange held back '
                             'to the last micro-batch' % world)
        if getattr(configs, 'share_videos', False):
            raise ValueError('--accum_steps > 1 with --share_videos is refused: the shared step accumulates at the library and Engine level only '
                             '(Engine.backward(accumulate=True))')
    return accum


def rank_of(configs, world=1):
    """--rank_negatives / --rank_lambda / --rank_temperature / --rank_relevance -> (n, lambda, temperature, relevance), or None (off; a configs.json from
    before the flags has none).  The three options belong to --rank_negatives and are refused without it; in --mode train, n > 0 needs
    --share_videos, --data resident, --optimizer fused and --accum_steps 1 (--mode test only reads what the run stored)."""
    n = int(getattr(configs, 'rank_negatives', 0) or 0)
    lam, temp, rel = (getattr(configs, k, None) for k in ('rank_lambda', 'rank_temperature', 'rank_relevance'))
    if n < 0:
        raise ValueError('--rank_negatives %d: at least 0 (0: off)' % n)
    if n == 0:
        for flag, v in (('--rank_lambda', lam), ('--rank_temperature', temp), ('--rank_relevance', rel)):
            if v is not None:
                raise ValueError('%s needs --rank_negatives n > 0: it belongs to the video ranking loss' % flag)
        return None
    lam, temp, rel = 1.0 if lam is None else float(lam), 0.1 if temp is None else float(temp), rel or 'max'
    if not temp > 0:
        raise ValueError('--rank_temperature %g: must be positive' % temp)
    if rel not in ('max', 'mean'):
        raise ValueError('--rank_relevance %r: max or mean' % (rel,))
    if configs.mode.lower() == 'train':
        if not getattr(configs, 'share_videos', False):
            raise ValueError('--rank_negatives needs --share_videos: the negative rows are the same query against other videos of the step, which the shared step encodes once')
        if configs.data != 'resident':
            raise ValueError('--rank_negatives needs --data resident (the sampler gathers the step\'s videos out of the split held in device memory)')
        if configs.optimizer != 'fused':
            raise ValueError('--rank_negatives needs --optimizer fused (the step runs through the engine: forward_shared, group_loss, fused backward)')
        if int(getattr(configs, 'accum_steps', 1) or 1) != 1:
            raise ValueError('--rank_negatives needs --accum_steps 1: the ranking step does not accumulate')
        if world > 1:
            raise ValueError('--rank_negatives is single-process (world = %d): data parallel through a shared encoding is not supported' % world)
        if 1 + n > int(configs.batch_size):
            raise ValueError('--rank_negatives %d: a group of %d rows does not fit into --batch_size %d rows' % (n, 1 + n, configs.batch_size))
    return n, lam, temp, rel


def check_corpus(configs):
    """--corpus in --mode test and what it needs (a configs.json from before the flag has none; --mode train only stores the flag)"""
    if not getattr(configs, 'corpus', False) or configs.mode.lower() != 'test':
        return False
    if configs.data != 'resident':
        raise ValueError('--corpus needs --data resident (every video of the split is encoded in device memory)')
    if topk_of(configs) is None:
        raise ValueError('--corpus needs --topk K >= 1: the moments returned per query')
    return True


def prefilter_of(configs):
    """--corpus_prefilter / --corpus_relevance -> (M, relevance); both belong to --corpus and are refused without it (a configs.json from before the
    flags has none: the defaults)"""
    m = int(getattr(configs, 'corpus_prefilter', 0) or 0)
    relevance = getattr(configs, 'corpus_relevance', None) or 'max'
    if m < 0:
        raise ValueError('--corpus_prefilter %d: at least 0 (0: every video)' % m)
    if relevance not in ('max', 'mean'):
        raise ValueError('--corpus_relevance %r: max or mean' % (relevance,))
    if (m or relevance != 'max') and not getattr(configs, 'corpus', False):
        raise ValueError('--corpus_prefilter / --corpus_relevance need --corpus: they choose how the corpus search runs')
    return m, relevance


def window_of(configs):
    """--window / --window_stride in --mode test -> (window, stride), or None (off; a configs.json from before the flags has none; --mode train only stores them)"""
    window = int(getattr(configs, 'window', 0) or 0)
    if window == 0 or configs.mode.lower() != 'test':
        return None
    stride = int(getattr(configs, 'window_stride', 0) or 0) or max(1, window // 2)
    if configs.data != 'resident':
        raise ValueError('--window needs --data resident (the windows run over the split held in device memory)')
    if not 1 <= window <= int(configs.max_pos_len):
        raise ValueError('--window %d: between 1 and --max_pos_len %d (the model has a positional row per clip of a window)' % (window, configs.max_pos_len))
    if not 1 <= stride <= window:
        raise ValueError('--window_stride %d: between 1 and --window %d (a larger stride would skip clips)' % (stride, window))
    return window, stride


def topk_of(configs):
    """--topk / --nms_iou / --max_span -> the `topk` argument of the evaluation loops (None: off; a configs.json from before the flags has none)"""
    k = int(getattr(configs, 'topk', 0) or 0)
    if k == 0:
        return None
    if not 1 <= k <= 32:
        raise ValueError('--topk %d: between 1 and 32 (0: off)' % k)
    nms_iou, max_span = float(getattr(configs, 'nms_iou', 0.5)), int(getattr(configs, 'max_span', 0) or 0)
    if not 0.0 <= nms_iou <= 1.0:
        raise ValueError('--nms_iou %g: between 0 and 1' % nms_iou)
    if max_span < 0:
        raise ValueError('--max_span %d: at least 0 (0: unlimited)' % max_span)
    return runner.TopK(k, nms_iou, max_span)


def train(configs, dataset, features, device, world, rank, log=print):
    from vslnet_amd.model.VSLNet import VSLNet, build_optimizer_and_scheduler
    model_dir = model_home(configs)
    accum = check_accum(configs, world)
    topk = topk_of(configs)
    rank_loss = rank_of(configs, world)
    if rank_loss is not None:                                               # (the resolved values go into configs.json)
        configs.rank_negatives, configs.rank_lambda, configs.rank_temperature, configs.rank_relevance = rank_loss
    gen = torch.Generator().manual_seed(configs.seed)                       # same shuffle on every rank
    share = bool(getattr(configs, 'share_videos', False))
    if share:
        if world > 1:
            raise ValueError('--mode train --share_videos is single-process: data parallel through a shared encoding is not supported (run without torchrun)')
        if configs.data != 'resident':
            raise ValueError('--mode train --share_videos needs --data resident (the grouped order gathers one feature row per video out of the split held in device memory)')
        if configs.optimizer != 'fused':
            raise ValueError('--mode train --share_videos runs the production sequence (lazy loss, fused optimizer): use --optimizer fused')
    if configs.data == 'resident':
        train_loader = data.ResidentSplit(dataset['train_set'], features, configs, device, train=True, generator=gen)
        test_loader = data.ResidentSplit(dataset['test_set'], features, configs, device, train=False)
        shards = (lambda: train_loader.shards(queries_per_video=configs.queries_per_video)) if share else (lambda: train_loader.shards(rank, world, micro_batches=accum))
        if rank_loss is not None:
            shards = lambda: train_loader.shards(negatives=rank_loss[0])
        log('dataset resident in HBM: %.1f MiB train, %.1f MiB test' % (train_loader.nbytes() / 2 ** 20, test_loader.nbytes() / 2 ** 20))
    elif configs.data == 'loader':
        train_loader = data.get_train_loader(dataset['train_set'], features, configs, pin=True, generator=gen)
        test_loader = data.get_test_loader(dataset['test_set'], features, configs, pin=True)
        shards = lambda: data.loader_shards(train_loader, device, rank, world, micro_batches=accum)
    else:
        raise ValueError('Unknown --data {}!!!'.format(configs.data))
    n_batches = len(train_loader) if rank_loss is None else train_loader.steps_per_epoch(rank_loss[0])     # (batch_size // (1 + n) queries per step)
    configs.num_train_steps = n_batches * configs.epochs                    # main_t7.py:58
    if rank == 0:
        os.makedirs(model_dir, exist_ok=True)
        with open(os.path.join(model_dir, 'configs.json'), 'w', encoding='utf-8') as f:
            f.write(json.dumps(vars(configs), indent=4, sort_keys=True))
    model = VSLNet(configs=configs, word_vectors=dataset['word_vector']).to(device)
    fused = configs.optimizer == 'fused'
    if not fused and world > 1:
        raise ValueError('--optimizer torch is single-process; use --optimizer fused under torch.distributed.run')
    if fused:
        flat, grads = model.flat_parameters
        eng = model._engine
        opt = dp.FlatAdamW(flat, eng.layout, lr=configs.init_lr, num_train_steps=configs.num_train_steps,
                           warmup_proportion=configs.warmup_proportion, clip_norm=configs.clip_norm, engine=eng,
                           hf_order=configs.adamw == 'hf')
        pad_vec, glove_vec = model.embedding_net.word_emb.pad_vec.data, model.embedding_net.word_emb.glove_vec.data
        # N > 1: backward + exchange as bench.py runs it -- the predictor block of the bucket goes out on a side stream behind the library's
        # early-gradient event while the rest of the backward runs (dp.OverlappedExchange); VSL_ALLREDUCE=single: one call behind the backward
        xchg = dp.OverlappedExchange(eng) if world > 1 and os.environ.get('VSL_ALLREDUCE', 'overlap') != 'single' else None
    else:
        optimizer, scheduler = build_optimizer_and_scheduler(model, configs)
    eval_period = max(1, n_batches // 2)
    best_r1i7, global_step, history = -1.0, 0, []
    score_writer = open(os.path.join(model_dir, 'eval_results.txt'), 'w', encoding='utf-8') if rank == 0 else None
    ckpt = runner.CheckpointWriter(device) if rank == 0 else None      # main_t7.py:125-126 without stalling the step
    log('start training...')
    # VSL_E2E_TRACE=1: host-side seconds per phase of the loop (tools/e2e_rate.py prints them): what the CLI adds around the bench step
    trace = {'batch': 0.0, 'step_enqueue': 0.0, 'log': 0.0, 'eval': 0.0, 'checkpoint': 0.0} if os.environ.get('VSL_E2E_TRACE') == '1' else None
    if os.environ.get('VSL_E2E_TRACE') == '2':            # attribution run: synchronise at every phase boundary (serialises host and GPU)
        trace = {'batch': 0.0, 'step_enqueue': 0.0, 'log': 0.0, 'eval': 0.0, 'checkpoint': 0.0}

        def clock():
            torch.cuda.synchronize()
            return time.perf_counter()
    else:
        clock = time.perf_counter
    epoch_end = []                                                         # wall clock at the end of every epoch (device idle)
    try:
        for epoch in range(configs.epochs):
            model.train()
            it = iter(shards() if fused else train_loader)
            while True:
                t0 = clock()
                try:
                    batch = next(it)
                except StopIteration:
                    break
                # --accum_steps K: the K pieces of this global batch (one draw of the order); pieces without rows are skipped
                micro = [batch] if accum == 1 else [b for b in [batch] + [next(it) for _ in range(accum - 1)] if b['vfeats'].shape[0]]
                t1 = clock()
                if trace is not None:
                    trace['batch'] += t1 - t0
                global_step += 1
                if fused:
                    # this rank's rows, padded to the GLOBAL batch widths; the losses are normalised with the global batch
                    inv_batch, mask_sum = dp.global_normalisers(batch['lens_global'])
                    parts, rank_log = [], None
                    for j, batch in enumerate(micro):
                        if rank_loss is not None:       # the video ranking step: groups of rows, the loss as two launches of its own (never lazy)
                            eng.forward_shared(flat, pad_vec, glove_vec, batch['word_ids'], batch['char_ids'], batch['vfeats'], batch['video_v_mask'],
                                               (batch['word_ids'] != 0).float(), batch['video_index'], training=True, seed=(configs.seed << 20) + global_step)
                            gl, hits, _, *seeds = eng.group_loss(batch['s_labels'], batch['e_labels'], batch['h_labels'], batch['group_start'], batch['positive'],
                                                                 1.0, configs.highlight_lambda, rank_loss[1], rank_loss[2], rank_loss[3],
                                                                 inv_pos=1.0 / batch['n_pos'], inv_groups=1.0 / batch['n_pos'], mask_sum=mask_sum)
                            dp.backward_exchange_step(eng, xchg, grads, seeds, opt)
                            parts.append(gl[3])
                            rank_log = (gl, hits, batch['n_pos'])
                            continue
                        if batch['vfeats'].shape[0] == 0:
                            # a rank without rows in this batch: zero bucket, same exchange calls, same (replicated) update
                            losses, seeds = torch.zeros(4, device=device), None
                        else:
                            q_mask = (batch['word_ids'] != 0).float()
                            if share:       # N videos, B queries: the video half once per video (the engine's backward dispatches on the last forward)
                                eng.forward_shared(flat, pad_vec, glove_vec, batch['word_ids'], batch['char_ids'], batch['vfeats'], batch['video_v_mask'], q_mask,
                                                   batch['video_index'], training=True, seed=(configs.seed << 20) + global_step)
                            else:
                                eng.forward(flat, pad_vec, glove_vec, batch['word_ids'], batch['char_ids'], batch['vfeats'], batch['v_mask'], q_mask,
                                            training=True, seed=(configs.seed << 20) + global_step, sample_offset=batch['row0'])
                            losses, *seeds = eng.loss(batch['s_labels'], batch['e_labels'], batch['h_labels'], 1.0,
                                                      configs.highlight_lambda, inv_batch=inv_batch, mask_sum=mask_sum, lazy=True)
                        if accum == 1:
                            dp.backward_exchange_step(eng, xchg, grads, seeds, opt)          # (tests/test_dp_gloo.py drives its multi-rank half on 2 and 3 ranks)
                        else:       # the first piece overwrites the bucket, the others add to it, the last one applies the step to the sum
                            dp.backward_exchange_step(eng, xchg, grads, seeds, opt, accumulate=j > 0, update=j == len(micro) - 1)
                        parts.append(losses[2])
                    # (the pieces' losses are partial sums of the global loss, as across ranks: added only when the step is logged)
                    loss_t = parts[0] if len(parts) == 1 else parts
                else:
                    _, vfeats, vfeat_lens, word_ids, char_ids, s_labels, e_labels, h_labels = batch
                    vfeats, vfeat_lens, word_ids, char_ids, s_labels, e_labels, h_labels = _to_device(
                        [vfeats, vfeat_lens, word_ids, char_ids, s_labels, e_labels, h_labels], device)
                    query_mask = (word_ids != 0).float()
                    video_mask = runner.convert_length_to_mask(vfeat_lens)
                    h_score, start_logits, end_logits = model(word_ids, char_ids, vfeats, video_mask, query_mask)
                    highlight_loss = model.compute_highlight_loss(h_score, h_labels, video_mask)
                    loc_loss = model.compute_loss(start_logits, end_logits, s_labels, e_labels)
                    loss_t = loc_loss + configs.highlight_lambda * highlight_loss
                    optimizer.zero_grad()
                    loss_t.backward()
                    torch.nn.utils.clip_grad_norm_(model.parameters(), configs.clip_norm)
                    optimizer.step()
                    scheduler.step()
                t2 = clock()
                if trace is not None:
                    trace['step_enqueue'] += t2 - t1
                if global_step % configs.period == 0 or global_step == 1:
                    lv = float((torch.stack(loss_t).sum() if isinstance(loss_t, list) else loss_t).item())
                    if world > 1:                                   # local partial sums of the global loss
                        t = torch.tensor([lv], device=device)
                        torch.distributed.all_reduce(t)
                        lv = float(t.item())
                    history.append((global_step, lv))
                    if fused and rank_log is not None:
                        log('step %6d | loss %.4f | rank %.4f | hits %d/%d' % (global_step, lv, float(rank_log[0][2].item()), int(rank_log[1].item()), rank_log[2]))
                    else:
                        log('step %6d | loss %.4f' % (global_step, lv))
                t3 = clock()
                if trace is not None:
                    trace['log'] += t3 - t2
                if global_step % eval_period == 0 or global_step % n_batches == 0:
                    rank0_error = None
                    if rank == 0:
                        # Whatever rank 0 raises here -- the evaluation, or a failed write of an EARLIER checkpoint that save_flat re-raises at its
                        # entry -- is kept until every rank has agreed on it below: leaving the loop now would leave the other ranks in the
                        # all-reduce until the communicator times out.
                        try:
                            model.eval()
                            r1i3, r1i5, r1i7, mi, score_str, *rank_k = runner.eval_test(model, test_loader, device, 'test', epoch + 1, global_step, topk=topk)
                            t4 = clock()
                            if trace is not None:
                                trace['eval'] += t4 - t3
                            log('Epoch: %2d | Step: %5d | r1i3: %.2f | r1i5: %.2f | r1i7: %.2f | mIoU: %.2f' % (epoch + 1, global_step, r1i3, r1i5, r1i7, mi))
                            if rank_k:
                                log('                         | rank@%(k)d i3: %(r_k_i3).2f | i5: %(r_k_i5).2f | i7: %(r_k_i7).2f | best-of-%(k)d mIoU: %(mIoU_k).2f' % rank_k[0])
                            score_writer.write(score_str)
                            score_writer.flush()
                            history.append((global_step, dict({'r1i3': r1i3, 'r1i5': r1i5, 'r1i7': r1i7, 'mIoU': mi}, **(rank_k[0] if rank_k else {}))))
                            if r1i7 >= best_r1i7:
                                best_r1i7 = r1i7
                                ckpt.save_flat(model, os.path.join(model_dir, '{}_{}.t7'.format(configs.model_name, global_step)), model_dir,
                                               suffix='t7', max_to_keep=3)
                                if trace is not None:
                                    trace['checkpoint'] += clock() - t4
                            model.train()
                        except Exception as e:                                 # noqa: BLE001
                            if world == 1:
                                raise
                            rank0_error = e
                    if world > 1:
                        # agree on rank 0's state BEFORE the barrier (run on every rank, unconditionally)
                        bad = rank == 0 and (rank0_error is not None or (ckpt is not None and ckpt.err is not None))
                        failed = torch.tensor([1 if bad else 0], device=device)
                        torch.distributed.all_reduce(failed)
                        if int(failed.item()):
                            if rank == 0:
                                if rank0_error is not None:
                                    raise rank0_error
                                ckpt._raise_pending()
                            raise RuntimeError('rank 0 failed during evaluation / checkpointing; stopping every rank')
                        torch.distributed.barrier()
            torch.cuda.synchronize(device)
            epoch_end.append(time.perf_counter())
    finally:
        # an exception or Ctrl-C must not leave the writer thread mid-file: every queued checkpoint is written (atomically) first
        if score_writer:
            score_writer.close()
        if ckpt is not None:
            in_flight = sys.exc_info()[1]
            try:
                ckpt.close()                                               # every checkpoint is on disk when train() returns
            except Exception as e:                                         # noqa: BLE001
                if in_flight is None:
                    raise
                log('checkpoint writer failed while another error was in flight: %r' % (e,))      # keep the original exception
    return {'history': history, 'model_dir': model_dir, 'steps': global_step, 'trace': trace, 'epoch_end': epoch_end}


def test(configs, parser, argv, dataset, features, device, log=print):
    from vslnet_amd.model.VSLNet import VSLNet
    model_dir = model_home(configs)
    if not os.path.exists(model_dir):
        raise ValueError('No pre-trained weights exist')
    with open(os.path.join(model_dir, 'configs.json'), encoding='utf-8') as f:
        parser.set_defaults(**json.load(f))                                    # main_t7.py:136-138
    configs = parser.parse_args(argv)
    rank_loss = rank_of(configs)
    given = any(a == '--corpus_relevance' or a.startswith('--corpus_relevance=') for a in (sys.argv[1:] if argv is None else argv))
    if rank_loss is not None and getattr(configs, 'corpus', False) and not given:
        configs.corpus_relevance = rank_loss[3]                                # the relevance the run was trained to rank by
    model = VSLNet(configs=configs, word_vectors=dataset['word_vector']).to(device)
    model.load_state_dict(torch.load(runner.get_last_checkpoint(model_dir, suffix='t7'), map_location=device))
    model.eval()
    topk = topk_of(configs)
    check_corpus(configs)
    prefilter, relevance = prefilter_of(configs)
    windows = window_of(configs)
    if configs.data == 'resident':
        loader = data.ResidentSplit(dataset['test_set'], features, configs, device, train=False)
    else:
        loader = data.get_test_loader(dataset['test_set'], features, configs, pin=True)
    if getattr(configs, 'share_videos', False):
        if configs.data != 'resident':
            raise ValueError('--share_videos needs --data resident (the encoding is computed over the split held in device memory)')
        r1i3, r1i5, r1i7, mi, _, *rank_k = runner.eval_test_shared(model, loader, device, mode='test', topk=topk)
    else:
        r1i3, r1i5, r1i7, mi, _, *rank_k = runner.eval_test(model, loader, device, mode='test', topk=topk)
    rows = [('Rank@1, IoU=0.3', r1i3), ('Rank@1, IoU=0.5', r1i5), ('Rank@1, IoU=0.7', r1i7), ('mean IoU'.ljust(15), mi)]
    if rank_k:
        k = rank_k[0]['k']
        rows += [('Rank@%d, IoU=0.3' % k, rank_k[0]['r_k_i3']), ('Rank@%d, IoU=0.5' % k, rank_k[0]['r_k_i5']), ('Rank@%d, IoU=0.7' % k, rank_k[0]['r_k_i7']),
                 ('best-of-%d mean IoU' % k, rank_k[0]['mIoU_k'])]
    corpus = {}
    if getattr(configs, 'corpus', False):
        stats, _ = runner.eval_corpus(model, loader, device, topk, prefilter=prefilter, relevance=relevance)
        k = stats['k']
        if prefilter:
            rows += [('Prefilter (%s) video recall@%d' % (relevance, prefilter), stats['prefilter_recall_m'])]
        rows += [('Corpus Rank@%d, IoU=0.5' % k, stats['corpus_r_k_i5']), ('Corpus Rank@%d, IoU=0.7' % k, stats['corpus_r_k_i7']),
                 ('video Recall@%d' % k, stats['video_recall_k'])]
        corpus = {key: v for key, v in stats.items() if key != 'k'}
    if windows is not None:
        stats, _ = runner.eval_windows(model, loader, device, windows[0], windows[1], topk=topk)
        tag = 'Windows %d/%d ' % windows
        rows += [(tag + 'Rank@1, IoU=0.3', stats['win_r1i3']), (tag + 'Rank@1, IoU=0.5', stats['win_r1i5']), (tag + 'Rank@1, IoU=0.7', stats['win_r1i7']),
                 (tag + 'mean IoU', stats['win_mIoU'])]
        if topk is not None:
            rows += [(tag + 'Rank@%d, IoU=0.3' % topk.k, stats['win_r_k_i3']), (tag + 'Rank@%d, IoU=0.5' % topk.k, stats['win_r_k_i5']),
                     (tag + 'Rank@%d, IoU=0.7' % topk.k, stats['win_r_k_i7']), (tag + 'best-of-%d mean IoU' % topk.k, stats['win_mIoU_k'])]
        corpus = dict(corpus, **stats)
    for name, v in rows:
        log('\x1b[1;31m{}:\t{:.2f}\x1b[0m'.format(name, v))
    return dict({'r1i3': r1i3, 'r1i5': r1i5, 'r1i7': r1i7, 'mIoU': mi}, **(rank_k[0] if rank_k else {}), **corpus)


def run(argv=None, log=print):
    parser = build_parser()
    configs = parser.parse_args(argv)
    world, rank, local = _dist_env()
    rank_of(configs, world)                         # (before the dataset is built: a refused combination costs nothing)
    check_accum(configs, world)
    topk_of(configs)
    check_corpus(configs)
    prefilter_of(configs)
    window_of(configs)
    runner.set_th_config(configs.seed)
    dataset, features = data.load_dataset(configs)
    configs.char_size, configs.word_size = dataset['n_chars'], dataset['n_words']      # main_t7.py:52-53
    if not torch.cuda.is_available():
        raise RuntimeError('main.py needs an MI355X (ROCm device): the HIP path has no CPU fallback')
    device = torch.device('cuda', local if world > 1 else int(configs.gpu_idx or 0))
    torch.cuda.set_device(device)
    if world > 1 and not torch.distributed.is_initialized():
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        torch.distributed.init_process_group('nccl', device_id=device)
    quiet = (lambda *a, **k: None) if rank != 0 else log
    mode = configs.mode.lower()
    try:
        if mode == 'train':
            return train(configs, dataset, features, device, world, rank, quiet)
        if mode == 'test':
            return test(configs, parser, argv, dataset, features, device, quiet)
        raise ValueError('Unknown mode {}!!!'.format(configs.mode))
    finally:
        if world > 1 and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


if __name__ == '__main__':
    run(sys.argv[1:])
