#!/usr/bin/env python
"""Writes profiles/soft_batch_measured.txt: what soft-NMS for the images of a batch at once buys.

    python tools/measure_soft_batch.py [--out profiles/soft_batch_measured.txt]

1. The selection stage alone: B in {1, 4, 8, 16} images x 1000 rows, one class, building-sized boxes on a 1024^2 tile, the shipped
   config's score_thr, soft-NMS and max_per_img.  One call of kernels.multiclass_soft_nms_batched against the loop of
   LoftRoIHead.multiclass_nms image by image (the per-image path, which this work leaves as it is).  HIP events around each variant,
   the variants alternating in one process after a warm-up, median and min-max.  The condition: the batched median is no greater
   than the loop's at every B.
2. SceneDetector.run on the 4096^2 random scene of tools/measure_scene_batch.py (25 tiles, synthetic weights): the shipped soft-NMS
   at batch = 1 (the only way before) against batch = 2, 4, 8 with soft_nms_batched=True, and type='nms' at the same batches beside
   them; synchronised wall-clock, median and min-max, peak device memory.  No ratio is fixed in advance.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE, OVERLAP = 1024, 256
BATCHES = (1, 2, 4, 8)
STAGE_B = (1, 4, 8, 16)
ROWS = 1000


def events_round_robin(fns, reps, warm=2):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return ts


def wall_round_robin(fns, reps, warm=1):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def fmt(ts, w=8, p=1):
    return f'{statistics.median(ts):{w}.{p}f} ({min(ts):.{p}f}-{max(ts):.{p}f})'


def stage_inputs(B, seed):
    rng = np.random.RandomState(seed)
    xy = rng.uniform(0, TILE - 120, (B * ROWS, 2))
    wh = rng.uniform(20, 120, (B * ROWS, 2))
    bboxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    fg = rng.uniform(0, 1, B * ROWS).astype(np.float32)
    scores = np.stack([fg, 1 - fg], 1).astype(np.float32)
    return torch.from_numpy(bboxes).cuda(), torch.from_numpy(scores).cuda(), [b * ROWS for b in range(B + 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'soft_batch_measured.txt'))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--stage-reps', type=int, default=15)
    args = ap.parse_args()
    from bonai_amd import build, kernels as K
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from bonai_amd.loft.roi import LoftRoIHead
    from bonai_amd.scene import SceneDetector
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    rc = cfg.test_cfg.rcnn
    thr, nms, k = rc.score_thr, dict(rc.nms), rc.max_per_img
    lines = [f'# tools/measure_soft_batch.py, source hash {build.source_hash()}, {torch.cuda.get_device_name(0)}, one session',
             f'# 1. selection stage alone: B images x {ROWS} rows, C = 1, boxes of 20-120 px on a {TILE}^2 tile, score_thr {thr}, nms {nms},',
             f'#    max_per_img {k}.  batched = one kernels.multiclass_soft_nms_batched call; loop = LoftRoIHead.multiclass_nms per image.',
             f'#    HIP events, variants alternating in one process, 2 warm-up calls each, {args.stage_reps} timed: median (min-max) ms',
             '# B  | batched ms               | loop ms                  | loop / batched | detections (equal in both)']
    ok = True
    for B in STAGE_B:
        bboxes, scores, off = stage_inputs(B, 100 + B)
        out = {}

        def batched():
            out['b'] = K.multiclass_soft_nms_batched(bboxes, scores, off, thr, nms, k)

        def loop():
            out['l'] = [LoftRoIHead.multiclass_nms(None, bboxes[a:e], scores[a:e], thr, nms, k) for a, e in zip(off, off[1:])]
        ts = events_round_robin({'batched': batched, 'loop': loop}, args.stage_reps)
        counts = out['b'][2].tolist()
        same = counts == [int(d.shape[0]) for d, _ in out['l']] and all(
            torch.equal(out['b'][0][i, :n], d) and torch.equal(out['b'][1][i, :n], l) for i, (n, (d, l)) in enumerate(zip(counts, out['l'])))
        if not same:
            raise SystemExit(f'B = {B}: the batched selection differs from the per-image loop')
        mb, ml = statistics.median(ts['batched']), statistics.median(ts['loop'])
        ok = ok and mb <= ml
        lines.append(f'{B:4d} | {fmt(ts["batched"], 8, 3):24s} | {fmt(ts["loop"], 8, 3):24s} | {ml / mb:14.2f} | {sum(counts)}')
    lines.append('condition (batched median <= loop median at every B): ' + ('holds' if ok else 'FAILS'))

    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({kk: synth_tensor(kk, v.shape) for kk, v in m.state_dict().items()})
    m = m.cuda().eval()
    rcnn = m.roi_head.test_cfg
    soft, hard = rcnn.nms, type(rcnn.nms)(type='nms', iou_threshold=rcnn.nms.get('iou_threshold', 0.5))
    soft_dets = {1: SceneDetector(m, tile=TILE, overlap=OVERLAP)}
    soft_dets.update({b: SceneDetector(m, tile=TILE, overlap=OVERLAP, batch=b, soft_nms_batched=True) for b in BATCHES[1:]})
    rcnn.nms = hard
    hard_dets = {b: SceneDetector(m, tile=TILE, overlap=OVERLAP, batch=b) for b in BATCHES}
    g = torch.Generator().manual_seed(1)
    scene = (torch.randn(4096, 4096, 3, generator=g) * 58 + 120).clamp(0, 255).to(torch.uint8).cuda()
    last = {}

    def with_nms(nms_cfg, det, key):
        def call():
            rcnn.nms = nms_cfg
            try:
                last[key] = det.run(scene)
            finally:
                rcnn.nms = hard
        return call
    runs = {}
    for b in BATCHES:
        runs[f'soft_nms batch {b}'] = with_nms(soft, soft_dets[b], ('soft', b))
        runs[f'nms      batch {b}'] = with_nms(hard, hard_dets[b], ('hard', b))
    ts = wall_round_robin(runs, args.reps)
    lines += ['# 2. SceneDetector.run, 4096^2 random scene, 25 tiles, synthetic weights (detection counts say nothing about trained weights;',
              f'#    max_per_img = {rcnn.max_per_img}), tile {TILE}, overlap {OVERLAP}.  soft_nms batch 1 = the shipped config on the per-tile path;',
              '#    soft_nms batch > 1 = soft_nms_batched=True.  Variants alternating in one process, 1 warm-up run each, then',
              f'#    {args.reps} synchronised wall-clock runs: median (min-max) ms; peak = torch.cuda.max_memory_allocated of one run, MiB',
              '# variant           | run() ms                 | peak MiB | buildings kept']
    for name, fn in runs.items():
        key = ('soft' if name.startswith('soft') else 'hard', int(name.split()[-1]))
        lines.append(f'{name:19s} | {fmt(ts[name]):24s} | {peak_mib(fn):8.0f} | {len(last[key])}')
    base = statistics.median(ts['soft_nms batch 1'])
    lines.append('run() relative to soft_nms batch 1: ' + ', '.join(f'{n.replace("      ", " ")} x{statistics.median(t) / base:.3f}' for n, t in ts.items()))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
