#!/usr/bin/env python
"""Entry point with the argv surface of the reference's tools/test.py:17-67 for the LOFT hot path.

    python tools/test.py CONFIG [CHECKPOINT] [--out results.pkl] [--eval] [--ann-file F --img-prefix D] [--num N] [--tta h,v,r90]
                         [--fused-rle] [--footprints] [--coco-ap]

Dataset mode (the annotation file of ``cfg.data.test`` -- or ``--ann-file`` -- exists): every image of the file goes through
`model(return_loss=False, rescale=True, img=[...], img_metas=[[...]])` with samples_per_gpu = 1 (apis/test.py:26,53-72), results
are the reference's 3-tuples (bbox_results, segm_results as COCO RLE, offset_results) and ``--out`` pickles the list exactly as
single_gpu_test returns it.  ``--eval`` evaluates on the spot what the reference evaluates from that pickle with
tools/bonai/bonai_evaluation.py: roof / footprint F1 at IoU 0.5 and the offset aEPE / aAE of the footprint pairs
(bonai_amd/evaluation.py; footprints = roof bitmaps translated by the predicted offset, on the device).
``--fused-rle`` encodes the RLE strings straight from the mask logits (bonai_amd/csrc/mask_rle.hip: the same bytes, no full-image
bitmaps); ``--footprints`` also appends the footprints' RLE dicts (roof read through the rounded offset) as a fourth tuple element.
``--coco-ap`` (with ``--eval``) adds the COCO bbox / segm AP of CocoDataset.evaluate (bonai_amd/coco_eval.py: COCOeval restated on
the device, not run against pycocotools): COCOeval.summarize's lines, and the ``bbox_mAP`` ... keys in what ``--eval`` prints.
Without dataset files (offline, as in this image) or with ``--synthetic`` the inputs are seeded synthetic tiles.
"""
import argparse
import json
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bonai_amd.validate import run_dataset  # noqa: E402,F401  (the loop lives in the library: the trainer validates with it too)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('config')
    ap.add_argument('checkpoint', nargs='?')
    ap.add_argument('--out')
    ap.add_argument('--eval', action='store_true', help='roof / footprint F1 and offset aEPE / aAE (tools/bonai/bonai_evaluation.py)')
    ap.add_argument('--ann-file', help='annotation file (default: cfg.data.test.ann_file)')
    ap.add_argument('--img-prefix', help='tile directory (default: cfg.data.test.img_prefix)')
    ap.add_argument('--score-thr', type=float, default=0.4, help='evaluation: detections below are dropped (bonai_evaluation.py:30)')
    ap.add_argument('--min-area', type=float, default=500, help='evaluation: roofs smaller than this many pixels are dropped (:31)')
    ap.add_argument('--tta', help="test-time augmentation views, a comma-separated subset of h,v,r90,r180,r270 (overrides the "
                                  "MultiScaleFlipAug entry of cfg.data.test.pipeline); flips mirror the reference, rotations and "
                                  "the merged offsets are extensions")
    ap.add_argument('--synthetic', action='store_true')
    ap.add_argument('--num', type=int, default=4, help='synthetic mode: number of tiles')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--bitmap-masks', action='store_true',
                    help='synthetic mode: full-image bool masks like simple_test; default: COCO RLE dicts, i.e. what the reference\'s '
                         'single_gpu_test hands on after encode_mask_results (apis/test.py:59-67), encoded from the device')
    ap.add_argument('--fused-rle', action='store_true',
                    help='COCO RLE strings encoded on the device from the mask logits, without pasting full-image bitmaps (same bytes); '
                         'not with --eval or --bitmap-masks, which need the bitmaps')
    ap.add_argument('--footprints', action='store_true',
                    help='results become 4-tuples: the footprint masks (roof shifted by the rounded offset) as RLE dicts in the layout of '
                         'the segm results; implies --fused-rle')
    ap.add_argument('--coco-ap', action='store_true',
                    help='with --eval: COCO bbox / segm AP as the reference\'s CocoDataset.evaluate reports it (needs the pasted '
                         'bitmaps: not with --fused-rle / --footprints)')
    args = ap.parse_args()
    if args.coco_ap and not args.eval:
        ap.error('--coco-ap adds COCO AP to what --eval reports: give --eval too')
    if args.footprints:
        args.fused_rle = True
    if args.fused_rle and args.coco_ap:
        ap.error('--coco-ap computes segm AP on the pasted bitmaps, --fused-rle / --footprints build none: drop one of the two')
    if args.fused_rle and args.eval:
        ap.error('--fused-rle / --footprints build no mask bitmaps, --eval pairs buildings on them: drop one of the two')
    if args.fused_rle and args.bitmap_masks:
        ap.error('--fused-rle / --footprints return RLE dicts, --bitmap-masks asks for full-image bool masks: drop one of the two')
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    cfg = Config.fromfile(args.config)
    torch.manual_seed(0)
    if cfg.get('fp16'):                                    # tools/test.py:104-106 wrap_fp16_model
        from bonai_amd import lib as L
        L.set_act16(torch.float16)
    tcfg = (cfg.data.get('test') if cfg.get('data') else None) or {}
    ann = args.ann_file or tcfg.get('ann_file')
    prefix = args.img_prefix if args.img_prefix is not None else tcfg.get('img_prefix', '')
    files = [ann] if isinstance(ann, str) else list(ann or [])
    dataset_mode = not args.synthetic and files and all(os.path.exists(f) for f in files)
    if not dataset_mode and not args.bitmap_masks:
        cfg.test_cfg.rcnn['rle_masks'] = True
    if args.fused_rle:
        cfg.test_cfg.rcnn['rle_masks'] = 'fused'
        cfg.test_cfg.rcnn['footprint_rle'] = args.footprints
    from bonai_amd import tta
    tile = tuple(tcfg.get('img_scale', (1024, 1024)))[::-1] if dataset_mode else (args.size, args.size)
    views = tta.parse_tta_arg(args.tta, tile) if args.tta else tta.views_from_pipeline(tcfg.get('pipeline'), tile)
    if views is not None and len(views) == 1:
        views = None
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    if args.checkpoint:
        from bonai_amd.checkpoint import load_checkpoint
        load_checkpoint(model, args.checkpoint, strict=True)
    model = model.cuda().eval()
    t0 = time.time()
    if dataset_mode:
        from bonai_amd import evaluation as E
        from bonai_amd.dataset import BonaiDataset
        extra = {k: tcfg[k] for k in ('bbox_type', 'mask_type', 'offset_coordinate', 'resolution', 'classes') if k in tcfg}
        resized = tta.resize_from_pipeline(tcfg.get('pipeline'), tile) or {}
        if resized:
            if args.tta:
                raise SystemExit('--tta together with a test pipeline that resizes is refused: a resized view together with flips or '
                                 'rotations is not supported')
            # rescale=True semantics: boxes, masks and -- with rescale_offsets -- offsets land in the source frame
            model.roi_head.test_cfg['rescale_offsets'] = True
            print(f"test pipeline resizes to {resized['resize']['img_scale']}: test_cfg.rcnn.rescale_offsets = True (offsets are "
                  'divided by the scale factor, like the boxes)', flush=True)
        ds = BonaiDataset(ann, prefix, test_mode=True, test_views=views, **resized, **extra)
        coco = None
        if args.coco_ap:
            from bonai_amd.coco_eval import CocoEvaluator
            coco = CocoEvaluator(ds, metrics=('bbox', 'segm'))
        results, records = run_dataset(model, ds, evaluate=args.eval, eval_kw=dict(score_thr=args.score_thr, min_area=args.min_area),
                                       coco=coco)
        torch.cuda.synchronize()
        print(f'{len(ds) / (time.time() - t0):.2f} img/s (decode + inference + mask paste + RLE' + (' + evaluation)' if args.eval else ')'))
        if args.eval:
            summary = E.summarize(records)
            if coco is not None:
                summary['coco'] = coco.summarize(log=print)
            print(json.dumps(summary, indent=1))
    else:
        if files and not args.synthetic:
            print(f'dataset files of cfg.data.test not found ({files[:1]}...): synthetic tiles', flush=True)
        results = []
        for i in range(args.num):
            data = make_batch(1, args.size, 40, step=i, device='cuda')
            imgs, metas = [data['img']], [data['img_metas']]
            if views is not None:                       # the views of the synthetic tile (a dataset builds them in one launch)
                from bonai_amd.data import d4_apply
                imgs = [torch.from_numpy(d4_apply(data['img'].cpu().numpy(), tta.view_element(v), axes=(2, 3)).copy()).cuda() for v in views]
                metas = [[tta.view_meta(data['img_metas'][0], v)] for v in views]
            with torch.no_grad():
                res = model(img=imgs, img_metas=metas, return_loss=False, rescale=True)
            results.append(res)
            print(f'[{i + 1}/{args.num}] dets={res[0][0].shape[0]} offsets={res[2].shape if hasattr(res[2], "shape") else 0}', flush=True)
        torch.cuda.synchronize()
        print(f'{args.num / (time.time() - t0):.2f} img/s (incl. mask paste + result encoding)')
    if args.out:
        with open(args.out, 'wb') as f:
            pickle.dump(results, f)


if __name__ == '__main__':
    main()
