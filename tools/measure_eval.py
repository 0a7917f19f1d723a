#!/usr/bin/env python
"""What the BONAI metric costs inside a training job, at tile size (1024^2, G = 80 ground-truth buildings rasterised by
kernels.poly2mask from bonai_amd.synth annotations):

  1. the metric part of evaluation.evaluate_image for one image -- both pairings' intersections, all areas, and their way to the
     host -- with kernels.mask_pair_counts (two launches, one read-back) against the evaluation._intersections loop and the
     separate ``flatten(1).sum(1).cpu()`` reads it replaces, on the same device bitmaps, for P ~ 100 and P ~ 1000 predictions;
  2. one validation pass (bonai_amd.validate.run_dataset with evaluation) over synthetic tiles with and without
     test_cfg.rcnn['paste_min_score'].

Host wall time of work that ends in a device synchronise (the loops are host-bound: that is the point), median / min / max, the
cases alternating inside every repetition after warm-up.

    python tools/measure_eval.py [--out profiles/eval_measured.txt] [--reps 15] [--pass-reps 3] [--tiles 2]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZE, G = 1024, 80


def _anns(seed):
    """G synthetic buildings inside the tile, none of the parser's special cases."""
    from bonai_amd.synth import synth_bonai_anns
    rng = np.random.RandomState(100 + seed)
    anns = []
    for a in synth_bonai_anns(seed=seed, n=4 * G, size=SIZE):
        x, y, w, h = a['bbox']
        if {'ignore', 'only_footprint'} & set(a) or a['iscrowd'] or a['category_id'] != 1 or a['area'] <= 0 or 'offset' not in a \
                or 'building_height' not in a or x < 45 or y < 45 or x + w > SIZE - 45 or y + h > SIZE - 45 or w < 24 or h < 24:
            continue
        anns.append(a)
    return [anns[i] for i in rng.permutation(len(anns))[:G]]


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ts):
    t = np.asarray(ts)
    return f'{np.median(t):9.3f} ms  (min {t.min():.3f}, max {t.max():.3f})'


def metric_part(P, reps, warmup, lines):
    from bonai_amd import evaluation as E, kernels as K
    from bonai_amd.data import parse_bonai_annotations
    ann = parse_bonai_annotations(dict(width=SIZE, height=SIZE, filename='t.png'), _anns(0))
    n_gt = len(ann['roof_masks'])
    rng = np.random.RandomState(P)
    src = rng.randint(0, n_gt, P)
    jit = rng.uniform(-6, 6, (P, 2))
    polys, boxes = [], np.zeros((P, 4), np.float32)
    for i, g in enumerate(src):                                # predictions: ground-truth roofs moved by a few pixels
        xy = np.asarray(ann['roof_masks'][g][0], np.float64).reshape(-1, 2) + jit[i]
        polys.append([xy.reshape(-1).tolist()])
        boxes[i] = (xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max())
    po = (np.asarray(ann['offsets'], np.float32)[src] + rng.normal(0, 2, (P, 2))).astype(np.float32)
    pm = K.poly2mask(polys, SIZE, SIZE)
    fp = K.mask_translate(pm, torch.from_numpy(po).cuda())
    g_roof, g_fp = K.poly2mask(ann['roof_masks'], SIZE, SIZE), K.poly2mask(ann['footprint_masks'], SIZE, SIZE)
    win = np.stack([np.floor(boxes[:, 0]) - 2, np.floor(boxes[:, 1]) - 2, np.ceil(boxes[:, 2]) + 2, np.ceil(boxes[:, 3]) + 2], 1)
    sh = np.sign(po) * np.floor(np.abs(po) + 0.5)
    win_fp = win - np.concatenate([sh, sh], 1)
    gb_roof, gb_fp = E.polygon_boxes(ann['roof_masks']), E.polygon_boxes(ann['footprint_masks'])

    def old():
        res = [pm.flatten(1).sum(1).cpu().numpy()]                                      # evaluate_image's area filter read
        for p_, g_, w_ in ((pm, g_roof, win), (fp, g_fp, win_fp)):
            res += [E._intersections(p_, g_, w_).cpu().numpy(), p_.flatten(1).sum(1).cpu().numpy(), g_.flatten(1).sum(1).cpu().numpy()]
        return res

    def new(cull=True):
        tabs = torch.from_numpy(np.concatenate([win, win_fp, gb_roof, gb_fp]).astype(np.int32)).cuda()
        m = P * n_gt + P + n_gt
        buf = torch.empty(2 * m, dtype=torch.int32, device='cuda')
        for k, (p_, g_) in enumerate(((pm, g_roof), (fp, g_fp))):
            K.mask_pair_counts(p_, g_, tabs[k * P:(k + 1) * P], tabs[2 * P + k * n_gt:2 * P + (k + 1) * n_gt] if cull else None,
                               out=buf[k * m:(k + 1) * m])
        h = buf.cpu().numpy()
        return [h[:P], *(x for k in range(2) for x in (h[k * m:k * m + P * n_gt].reshape(P, n_gt), h[k * m + P * n_gt:k * m + P * n_gt + P],
                                                       h[k * m + P * n_gt + P:(k + 1) * m]))]
    cases = [('_intersections loop + 7 read-backs (before)', old), ('mask_pair_counts x 2 + 1 read-back', new),
             ('mask_pair_counts x 2 + 1 read-back, no gbox', lambda: new(False))]
    want = old()
    for name, fn in cases[1:]:
        got = fn()
        assert all(np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64)) for a, b in zip(want[1:], got[1:])), name
    times = {name: [] for name, _ in cases}
    for rep in range(warmup + reps):
        for name, fn in cases:
            t, _ = _timed(fn)
            if rep >= warmup:
                times[name].append(t)
    lines.append(f'metric part of one image, P = {P} predictions x G = {n_gt} ground truths, {SIZE}^2 (results identical, checked):')
    for name, _ in cases:
        lines.append(f'  {name:50s} {_stats(times[name])}')
    return {name: float(np.median(t)) for name, t in times.items()}


def validation_pass(tiles, reps, lines):
    from PIL import Image
    from bonai_amd.config import Config
    from bonai_amd.dataset import BonaiDataset
    from bonai_amd.loft import build_detector
    from bonai_amd.validate import run_dataset
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg).cuda().eval()     # seeded random initialisation:
    # (an untrained model, i.e. the many-low-score-detections case an early validation pass meets)
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.RandomState(1)
        images, annotations, aid = [], [], 0
        for i in range(tiles):
            name = f'tile_{i}.png'
            Image.fromarray(rng.randint(0, 255, (SIZE, SIZE, 3)).astype(np.uint8)).save(os.path.join(d, name), compress_level=1)
            images.append(dict(id=i + 1, file_name=name, width=SIZE, height=SIZE))
            for a in _anns(i):
                aid += 1
                annotations.append(dict(a, id=aid, image_id=i + 1))
        f = os.path.join(d, 'val.json')
        json.dump(dict(images=images, annotations=annotations, categories=[dict(id=1, name='building')]), open(f, 'w'))
        ds = BonaiDataset(f, d, test_mode=True)
        rc = model.roi_head.test_cfg
        times, pasted = {None: [], 0.4: []}, {}
        for rep in range(1 + reps):
            for thr in (None, 0.4):
                rc.pop('paste_min_score', None)
                if thr is not None:
                    rc['paste_min_score'] = thr
                t, (results, _) = _timed(lambda: run_dataset(model, ds, evaluate=True, eval_kw=dict(score_thr=0.4), log=lambda *_: None))
                pasted[thr] = sum(b.shape[0] for r in results for b in r[0])
                if rep >= 1:
                    times[thr].append(t)
        rc.pop('paste_min_score', None)
    lines.append(f'one validation pass over {tiles} tiles of {SIZE}^2 (decode + inference + paste + RLE + evaluation), randomly initialised '
                 'model:')
    lines.append(f"  {'paste_min_score absent':30s} {_stats(times[None])}   {pasted[None]} detections pasted")
    lines.append(f"  {'paste_min_score = 0.4':30s} {_stats(times[0.4])}   {pasted[0.4]} detections pasted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--pass-reps', type=int, default=3)
    ap.add_argument('--tiles', type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    lines = [f'# BONAI metric at tile size; host wall time of work ending in a device synchronise, median (min, max) of {args.reps} calls',
             f'# after {args.warmup} warm-up ({args.pass_reps} passes after 1 for the validation pass), the cases alternating, one process, one session',
             f'# device {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]})']
    for P in (100, 1000):
        metric_part(P, args.reps, args.warmup, lines)
    if args.tiles > 0:
        validation_pass(args.tiles, args.pass_reps, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
