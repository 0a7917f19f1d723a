#!/usr/bin/env python
"""Entry point with the argv surface of the reference's tools/train.py:25-64 for the LOFT hot path.

    python tools/train.py configs/loft_foa/loft_foa_r50_fpn_2x_bonai.py [--work-dir D] [--launcher pytorch]
                          [--options k=v ...] [--iters N] [--synthetic] [--no-validate] [--val-ann-file F --val-img-prefix D]

Data: when the annotation files of ``cfg.data.train`` exist, batches come from them (bonai_amd/dataset.py: the reference's
BONAI dataset + train pipeline semantics, polygons rasterised and images normalised on the device), sharded over the ranks like
DistributedGroupSampler; otherwise -- offline, as in this image -- or with ``--synthetic``, seeded 1024x1024 tiles with the
reference's batch-dict keys.  Logging mirrors TextLoggerHook's key set (default_runtime.py:3-8).

Validation (the reference's EvalHook, apis/train.py:113-126): when the annotation files of ``cfg.data.val`` -- or ``--val-ann-file``
-- exist, every ``cfg.evaluation.interval``-th epoch ends with a pass over them (bonai_amd/validate.py: roof / footprint F1 and
offset aEPE / aAE, sharded over the ranks), an ``Epoch(val)`` line and a line in WORK_DIR/val.log.json; ``evaluation.save_best``
keeps best.pth.  ``evaluation.coco_ap=True`` (opt-in) also computes the COCO AP the config's ``metric=['bbox', 'segm']`` names
(bonai_amd/coco_eval.py): bbox_mAP / segm_mAP in the line, all keys in val.log.json, save_best='coco.segm_mAP'.  When batches come from annotation files, ``checkpoint_config.interval`` writes epoch_{E}.pth (a synthetic stream
has no epochs of its own: latest.pth only).  Validation runs uncaptured and is refused together with ``--graph``.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def parse_option(opt):
    """'key=value' -> (key, value): Python literals (numbers, tuples, lists, True/False/None, quoted strings) through
    ast.literal_eval -- never eval() --, anything else stays the string it is (mmcv DictAction's behaviour for plain words)."""
    import ast
    if '=' not in opt:
        raise ValueError(f'--options takes key=value pairs, got {opt!r}')
    k, v = opt.split('=', 1)
    try:
        return k, ast.literal_eval(v)
    except (ValueError, SyntaxError):
        return k, v


def optimizer_kwargs(cfg, model, options=(), verbose=False):
    """Trainer's optimizer arguments from cfg.optimizer (type, options, paramwise_cfg) and cfg.optimizer_config.grad_clip
    (bonai_amd/optim.py); needs no device.  ``--options optimizer.type=X`` over a config written for the other rule leaves that
    rule's own options behind (SGD's momentum under AdamW): those are dropped, and named on stdout."""
    from bonai_amd.optim import drop_foreign_options, trainer_kwargs
    if any(o.split('=', 1)[0] == 'optimizer.type' for o in options):
        kept, dropped = drop_foreign_options(cfg.optimizer)
        if dropped:
            cfg.optimizer = kept
            if verbose:
                print(f"optimizer.type={kept['type']} given on the command line: dropped the config's {dropped}", flush=True)
    return trainer_kwargs(cfg, model)


def augment_kwargs(pipeline):
    """BonaiDataset's augmentation arguments from the train pipeline: the RandomFlip entry (flip_ratio, direction) and the
    RandomRotate entry (rotate_ratio, choice), and which of the two stands first -- they do not commute."""
    names = [p.get('type') for p in pipeline]
    flip = next((p for p in pipeline if p.get('type') == 'RandomFlip'), {})
    kw = dict(flip_ratio=flip.get('flip_ratio', 0.0) or 0.0, flip_direction=flip.get('direction', 'horizontal'))
    if 'RandomRotate' in names:
        rot = pipeline[names.index('RandomRotate')]
        kw.update(rotate_ratio=rot.get('rotate_ratio'), rotate_choice=rot.get('choice', (0, 90, 180, 270)),
                  rotate_first='RandomFlip' in names and names.index('RandomRotate') < names.index('RandomFlip'))
    return kw


def resize_kwargs(pipeline, tile=(1024, 1024)):
    """BonaiDataset's ``resize`` / ``pad_divisor`` from the pipeline's Resize and Pad entries.  A Resize that is an identity on the
    dataset's tiles (one keep_ratio scale equal to the tile, no ratio_range) with a Pad divisor that divides the tile is passed as
    nothing at all: the loader then runs exactly as it did before Resize existed."""
    rs = next((p for p in pipeline if p.get('type') == 'Resize'), None)
    pad = next((p for p in pipeline if p.get('type') == 'Pad'), None)
    if pad is not None and pad.get('size') is not None:
        raise NotImplementedError("Pad(size=...) is not supported: give size_divisor")
    divisor = (pad or {}).get('size_divisor')
    if rs is not None:
        scales = rs.get('img_scale')
        scales = list(scales) if isinstance(scales, list) else [scales]
        identity = rs.get('ratio_range') is None and len(scales) == 1 and scales[0] is not None and \
            tuple(scales[0]) in (tuple(tile), tuple(tile)[::-1]) and rs.get('keep_ratio', True) and \
            not (divisor and (tile[0] % divisor or tile[1] % divisor))
        if not identity:
            return dict(resize={k: v for k, v in rs.items() if k != 'type'}, pad_divisor=divisor)
    return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('config')
    ap.add_argument('--work-dir')
    ap.add_argument('--resume-from', help='checkpoint written by this tool / the reference: weights, SGD momentum, iter, epoch')
    ap.add_argument('--load-from', help='weights only (apis/train.py:141-142)')
    ap.add_argument('--pretrained', help='local backbone checkpoint (torchvision / model-zoo keys) replacing cfg.model.pretrained')
    ap.add_argument('--iters-per-epoch', type=int, default=0, help='synthetic stream: iterations that count as one epoch (0: one epoch)')
    ap.add_argument('--launcher', choices=['none', 'pytorch'], default='none')
    ap.add_argument('--options', nargs='+', default=[])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--local_rank', type=int, default=0)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--synthetic', action='store_true', help='seeded synthetic tiles even when the dataset files are present')
    ap.add_argument('--prefetch', type=int, default=2, help='dataset batches decoded / uploaded ahead of the step (0: synchronous loader)')
    ap.add_argument('--graph', action='store_true', help='backbone + neck forward / backward as two hipGraphs (bonai_amd/graphs.py)')
    ap.add_argument('--no-validate', action='store_true', help='no validation pass at epoch ends (tools/train.py:36-39 of the reference)')
    ap.add_argument('--val-ann-file', help='validation annotation file (default: cfg.data.val.ann_file)')
    ap.add_argument('--val-img-prefix', help='validation tile directory (default: cfg.data.val.img_prefix)')
    args = ap.parse_args()
    from bonai_amd.config import Config
    from bonai_amd.engine import Trainer, step_lr
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    cfg = Config.fromfile(args.config)
    if args.options:
        cfg.merge_from_dict(dict(parse_option(o) for o in args.options))
    rank, world = 0, 1
    if args.launcher == 'pytorch':
        rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', args.local_rank)))
        dist.init_process_group(cfg.dist_params.get('backend', 'nccl'))
    torch.manual_seed(args.seed)
    from bonai_amd.checkpoint import load_checkpoint, save_checkpoint
    if cfg.get('fp16'):                # Fp16OptimizerHook recipe: half activations, fp32 masters; loss_scale: a number (the reference's
                                       # static scale), 'dynamic' or a dict (bonai_amd/loss_scale.py; --options fp16.loss_scale=dynamic)
        from bonai_amd import lib as L
        L.set_act16(torch.float16)
    if args.pretrained:
        cfg.model['pretrained'] = args.pretrained
    # validation: only when its annotation files are there (no existing invocation has them: nothing new runs then)
    vcfg = (cfg.data.get('val') if cfg.get('data') else None) or {}
    val_ann = args.val_ann_file or vcfg.get('ann_file')
    val_files = [val_ann] if isinstance(val_ann, str) else list(val_ann or [])
    validate = not args.no_validate and bool(val_files) and all(os.path.exists(f) for f in val_files)
    ev = None
    if validate:
        from bonai_amd.validate import parse_evaluation
        ev = parse_evaluation(cfg.get('evaluation'), log=(lambda m: print(m, flush=True)) if rank == 0 else (lambda m: None))
        if args.graph:
            raise SystemExit('--graph together with validation is refused: the validation pass runs uncaptured between two steps, and '
                             'that a captured backbone + neck step replays correctly after it has not been shown on the device.  '
                             'Give --no-validate, or train without --graph.')
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().train()
    if args.load_from:
        load_checkpoint(model, args.load_from, strict=False)
    tr = Trainer(model, **optimizer_kwargs(cfg, model, args.options, verbose=rank == 0),
                 loss_scale=(cfg.get('fp16') or {}).get('loss_scale', 1.0), graph_features=args.graph)
    start_iter = 0
    if args.resume_from:                                   # mmcv runner.resume: weights + optimizer state + iter / epoch
        ckpt = load_checkpoint(model, args.resume_from, strict=True)
        if ckpt.get('optimizer') is not None:
            tr.load_optimizer_state(ckpt['optimizer'])
        start_iter = int(ckpt.get('meta', {}).get('iter', 0))
    bs = cfg.data.get('samples_per_gpu', 8)
    interval = cfg.log_config.get('interval', 10)
    ipe = args.iters_per_epoch or max(args.iters, 1)
    sched = {k: cfg.lr_config[k] for k in ('warmup_iters', 'warmup_ratio', 'step') if k in cfg.lr_config}
    dataset = None
    tcfg = cfg.data.get('train') if cfg.get('data') else None
    if tcfg is not None and not args.synthetic:
        files = [tcfg['ann_file']] if isinstance(tcfg['ann_file'], str) else list(tcfg['ann_file'])
        if files and all(os.path.exists(f) for f in files):
            from bonai_amd.dataset import BonaiDataset
            extra = {k: tcfg[k] for k in ('offset_coordinate', 'resolution', 'ignore_buildings', 'filter_empty_gt', 'classes', 'img_scale')
                     if k in tcfg}                     # (bonai.py:18-35: the dataset's own keyword arguments)
            dataset = BonaiDataset(tcfg['ann_file'], tcfg.get('img_prefix', ''), bbox_type=tcfg.get('bbox_type', 'roof'),
                                   mask_type=tcfg.get('mask_type', 'roof'), seed=args.seed + rank,
                                   **augment_kwargs(tcfg.get('pipeline', [])),
                                   **resize_kwargs(tcfg.get('pipeline', []), tuple(tcfg.get('img_scale', (1024, 1024)))), **extra)
            if args.graph and dataset.multi_scale:
                raise SystemExit('--graph together with a Resize that can draw more than one size is refused: the captured backbone + '
                                 'neck graphs hold one input shape.  Train without --graph, or with a single img_scale.')
            ipe = args.iters_per_epoch or max(1, len(dataset.epoch_indices(0, bs, rank, world)) // bs)
        elif rank == 0:
            print(f'dataset files of cfg.data.train not found ({files[:1]}...): synthetic tiles', flush=True)

    def stream():
        if dataset is None:
            for it in range(start_iter, args.iters):
                yield it, make_batch(bs, 1024, 80, rank=rank, step=it, device='cuda')
            return
        it = start_iter
        while it < args.iters:
            for data in dataset.batches(it // ipe, bs, rank, world, seed=args.seed, prefetch=args.prefetch,
                                        workers=cfg.data.get('workers_per_gpu', 2) * 4):
                if it >= args.iters:
                    return
                yield it, data
                it += 1
    validator = None
    if validate:
        from bonai_amd.dataset import BonaiDataset
        from bonai_amd.validate import Validator, is_better, val_line
        vextra = {k: vcfg[k] for k in ('bbox_type', 'mask_type', 'offset_coordinate', 'resolution', 'classes') if k in vcfg}
        vprefix = args.val_img_prefix if args.val_img_prefix is not None else vcfg.get('img_prefix', '')
        validator = Validator(model, BonaiDataset(val_ann, vprefix, test_mode=True, **vextra), score_thr=ev['score_thr'],
                              min_area=ev['min_area'], iou_thr=ev['iou_thr'], rank=rank, world=world, num=ev['num'],
                              coco=ev.get('coco'))               # evaluation.coco_ap=True: COCO bbox / segm AP next to them
    ckpt_every = int((cfg.get('checkpoint_config') or {}).get('interval', 1) or 0)
    best = dict(value=None, epoch=None)

    def save(name, it_done, epoch, **meta):
        os.makedirs(args.work_dir, exist_ok=True)
        save_checkpoint(model, os.path.join(args.work_dir, name), optimizer_state=tr.optimizer_state_dict(),
                        meta=dict(config=cfg.filename, iter=it_done, epoch=epoch, **meta))

    def epoch_end(it_done, epoch):
        """After the last iteration of epoch ``epoch`` (1-based): validation, best checkpoint, epoch checkpoint."""
        if validator is not None and epoch % ev['interval'] == 0:
            summary = validator.run()                      # every rank runs its shard; all hold the same totals afterwards
            if rank == 0:
                print(val_line(epoch, validator.num, summary), flush=True)
                rec = dict(mode='val', epoch=epoch, iter=it_done, **summary)
                if ev['save_best']:
                    name, key = ev['save_best'].split('.', 1)
                    if is_better(ev['save_best'], summary[name][key], best['value']):
                        best.update(value=summary[name][key], epoch=epoch)
                        if args.work_dir:
                            save('best.pth', it_done, epoch, best={ev['save_best']: best['value']})
                    rec['best'] = dict(key=ev['save_best'], value=best['value'], epoch=best['epoch'])
                if args.work_dir:
                    os.makedirs(args.work_dir, exist_ok=True)
                    with open(os.path.join(args.work_dir, 'val.log.json'), 'a') as f:
                        f.write(json.dumps(rec) + '\n')
        if dataset is not None and args.work_dir and rank == 0 and ckpt_every > 0 and epoch % ckpt_every == 0:
            save(f'epoch_{epoch}.pth', it_done, epoch)

    t0 = time.time()
    for it, data in stream():
        out = tr.train_step(data, lr=step_lr(cfg.optimizer.lr, it, it // ipe, **sched))
        if rank == 0 and (it + 1) % interval == 0:
            torch.cuda.synchronize()
            lv = ', '.join(f'{k}: {v:.4f}' for k, v in out['log_vars'].items())
            if cfg.get('fp16'):                            # (log lines only: the one read-back of the loss scaler's device state)
                ls = tr.loss_scale_state()
                lv += f", loss_scale: {ls['scale']:g}, skipped: {ls['skipped']}, grad_norm: {ls['grad_norm']:.4f}"
            print(f'Epoch [{it // ipe + 1}][{it % ipe + 1}/{ipe}] time: {(time.time() - t0) / (it - start_iter + 1):.3f}, {lv}', flush=True)
        if (it + 1) % ipe == 0 and (validator is not None or dataset is not None):
            epoch_end(it + 1, (it + 1) // ipe)
    if args.work_dir and rank == 0:
        os.makedirs(args.work_dir, exist_ok=True)
        save_checkpoint(model, os.path.join(args.work_dir, 'latest.pth'), optimizer_state=tr.optimizer_state_dict(),
                        meta=dict(config=cfg.filename, iter=args.iters, epoch=args.iters // ipe))
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
