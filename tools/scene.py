#!/usr/bin/env python
"""Whole-scene inference: images of any size, cut into overlapping tiles on the device and merged on their masks
(bonai_amd/scene.py; an extension -- the reference's tools/bonai/bonai_test.py delegates this step to an external package).

    python tools/scene.py CONFIG [CHECKPOINT] IMAGE [IMAGE ...] --out results.pkl [--tile N] [--overlap N] [--merge-thr F]
                          [--footprints] [--batch N] [--hard-nms | --batched-soft-nms]

Images are decoded with PIL as the dataset decodes its tiles.  ``--out`` pickles one result tuple per image in simple_test's
layout for an image of the scene's size: (bbox_results, segm_results as COCO RLE, offset_results[, footprint RLE with --footprints]).
``--batch N`` (1 .. 16) sends the tiles through the model N at a time (LoftRoIHead.batch_test_device); it needs test_cfg.rcnn.nms of
type 'nms' -- soft-NMS is sequential per image -- and ``--hard-nms`` replaces the config's by type='nms' at the same iou_threshold;
``--batched-soft-nms`` instead keeps the config's soft-NMS and runs it for the tiles of a batch at once, one workgroup per tile
(kernels.multiclass_soft_nms_batched).  The two exclude each other.
A first positional argument after CONFIG that ends in .pth / .pt is the checkpoint; without one the weights are the seeded
initialisation (a smoke run).
"""
import argparse
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('config')
    ap.add_argument('paths', nargs='+', metavar='[CHECKPOINT] IMAGE', help='an optional checkpoint (.pth / .pt), then the images')
    ap.add_argument('--out', required=True)
    ap.add_argument('--tile', type=int, help='tile side, a multiple of 32 (default: cfg.data.test.img_scale, else 1024)')
    ap.add_argument('--overlap', type=int, default=256, help='pixels neighbouring tiles share at least')
    ap.add_argument('--merge-thr', type=float, default=0.5,
                    help='two detections of different tiles are one building when their masks share more than this part of the smaller')
    ap.add_argument('--footprints', action='store_true', help='results become 4-tuples: the footprints\' RLE dicts as well')
    ap.add_argument('--batch', type=int, default=1, help='tiles per pass through the model, 1 .. 16 (default 1: every tile alone)')
    ap.add_argument('--hard-nms', action='store_true',
                    help="test_cfg.rcnn.nms becomes type='nms' at the config's iou_threshold (--batch > 1 refuses soft-NMS)")
    ap.add_argument('--batched-soft-nms', action='store_true',
                    help="with --batch > 1 a type='soft_nms' config stays as it is and is selected for all tiles of a batch in one launch")
    args = ap.parse_args()
    if args.hard_nms and args.batched_soft_nms:
        ap.error('--batched-soft-nms keeps the soft-NMS of the config that --hard-nms replaces: give one of them')
    ckpt = args.paths[0] if args.paths[0].endswith(('.pth', '.pt')) else None
    images = args.paths[1:] if ckpt else args.paths
    if not images:
        ap.error('no image given')
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from bonai_amd.scene import SceneDetector, read_image
    cfg = Config.fromfile(args.config)
    torch.manual_seed(0)
    if args.hard_nms:
        cfg.test_cfg.rcnn.nms = dict(type='nms', iou_threshold=cfg.test_cfg.rcnn.nms.get('iou_threshold', 0.5))
    if cfg.get('fp16'):
        from bonai_amd import lib as L
        L.set_act16(torch.float16)
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    if ckpt:
        from bonai_amd.checkpoint import load_checkpoint
        load_checkpoint(model, ckpt, strict=True)
    model = model.cuda().eval()
    det = SceneDetector(model, tile=args.tile, overlap=args.overlap, merge_thr=args.merge_thr, footprints=args.footprints, cfg=cfg,
                        batch=args.batch, soft_nms_batched=args.batched_soft_nms)
    results = []
    for path in images:
        t0 = time.time()
        res = det.run(read_image(path))
        torch.cuda.synchronize()
        print(f'{path}: {res.size[1]}x{res.size[0]}, {len(res.origins)} tiles, {len(res)} buildings, {time.time() - t0:.2f} s', flush=True)
        results.append(res.as_result_tuple())
    with open(args.out, 'wb') as f:
        pickle.dump(results, f)


if __name__ == '__main__':
    main()
