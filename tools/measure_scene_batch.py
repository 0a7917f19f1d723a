#!/usr/bin/env python
"""Writes profiles/scene_batch_measured.txt: what sending the tiles of a scene through the model in batches buys.

    python tools/measure_scene_batch.py [--out profiles/scene_batch_measured.txt]

SceneDetector.run on the 4096^2 random scene of tools/measure_scene.py (25 tiles, synthetic weights, tile 1024, overlap 256) and on
the smallest load, a 1024^2 scene of one tile, with batch = 1, 2, 4 and 8: all of them alternating in one process after a warm-up
run of each, synchronised wall-clock, median and min-max; ``tile_detections`` (tiles through the model) timed apart from the merge;
peak device memory of a run.  batch > 1 needs test_cfg.rcnn.nms of type 'nms', the headline config ships soft-NMS: the yardstick is
batch = 1 with type='nms' -- today's per-tile path on the same detections -- and batch = 1 with the shipped soft-NMS is timed next to
it.  Also how far batch = 8 is from batch = 1 in results (kernel forms are chosen by problem size: bit-equality is not promised).
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE, OVERLAP = 1024, 256
BATCHES = (1, 2, 4, 8)


def timed_round_robin(fns, reps, warm=1):
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


def fmt(ts):
    return f'{statistics.median(ts):8.1f} ({min(ts):.1f}-{max(ts):.1f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_batch_measured.txt'))
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    from bonai_amd import build
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from bonai_amd.scene import SceneDetector
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    m = m.cuda().eval()
    rcnn = m.roi_head.test_cfg
    soft, hard = rcnn.nms, type(rcnn.nms)(type='nms', iou_threshold=rcnn.nms.get('iou_threshold', 0.5))
    shipped = SceneDetector(m, tile=TILE, overlap=OVERLAP)
    rcnn.nms = hard
    dets = {b: SceneDetector(m, tile=TILE, overlap=OVERLAP, batch=b) for b in BATCHES}
    g = torch.Generator().manual_seed(1)
    scene = (torch.randn(4096, 4096, 3, generator=g) * 58 + 120).clamp(0, 255).to(torch.uint8).cuda()
    last = {}

    def with_nms(nms, fn, key=None):
        def call():
            rcnn.nms = nms
            try:
                out = fn()
            finally:
                rcnn.nms = hard
            if key is not None:
                last[key] = out
        return call
    lines = [f'# tools/measure_scene_batch.py, source hash {build.source_hash()}, {torch.cuda.get_device_name(0)}, one session',
             f'# SceneDetector.run, synthetic weights (max_per_img = {rcnn.max_per_img}: detection counts say nothing about trained weights), tile',
             f'# {TILE}, overlap {OVERLAP}; every variant alternating in one process, 1 warm-up run each, then {args.reps} synchronised wall-clock',
             "# runs: median (min-max) ms.  batch = N: N tiles per pass through the model, test_cfg.rcnn.nms = dict(type='nms'); 'shipped' =",
             '# batch = 1 with the soft-NMS the config ships (batch > 1 refuses it).  tiles = tile_detections alone (cut + model, no merge);',
             '# peak = torch.cuda.max_memory_allocated of one run(), MiB (scene included).  The yardstick is batch = 1 of the same session.',
             '# scene      | variant  | run() ms                 | tiles ms                 | peak MiB | tiles | detections | kept']
    for name, sc in (('4096^2', scene), ('1024^2', scene[:TILE, :TILE].contiguous())):
        runs = {'shipped': with_nms(soft, lambda sc=sc: shipped.run(sc), ('run', 'shipped', name))}
        tiles = {'shipped': with_nms(soft, lambda sc=sc: shipped.tile_detections(sc), ('tiles', 'shipped', name))}
        for b, d in dets.items():
            runs[f'batch {b}'] = with_nms(hard, lambda d=d, sc=sc: d.run(sc), ('run', b, name))
            tiles[f'batch {b}'] = with_nms(hard, lambda d=d, sc=sc: d.tile_detections(sc), ('tiles', b, name))
        reps = args.reps if name == '4096^2' else 2 * args.reps
        t_run, t_tiles = timed_round_robin(runs, reps), timed_round_robin(tiles, reps)
        for k in runs:
            key = k if k == 'shipped' else int(k.split()[1])
            res, (origins, td) = last[('run', key, name)], last[('tiles', key, name)]
            lines.append(f'{name:12s} | {k:8s} | {fmt(t_run[k]):24s} | {fmt(t_tiles[k]):24s} | {peak_mib(runs[k]):8.0f} | {len(origins):5d} | '
                         f'{sum(int(d[0].shape[0]) for d in td):10d} | {len(res)}')
        base = statistics.median(t_run['batch 1'])
        lines.append(f'{name}: run() relative to batch 1: ' + ', '.join(f'{k} x{statistics.median(t_run[k]) / base:.3f}' for k in runs))
        if name == '1024^2':
            spread = max(t_run['batch 1']) - min(t_run['batch 1'])
            worst = max(statistics.median(t_run[f'batch {b}']) for b in BATCHES[1:]) - base
            lines.append(f'condition (one tile: batch > 1 costs no more than batch 1 beyond its spread of {spread:.2f} ms): worst median excess '
                         f'{worst:.2f} ms: ' + ('holds' if worst <= spread else 'FAILS'))
        else:
            a, b8 = last[('tiles', 1, name)][1], last[('tiles', 8, name)][1]
            ca, cb = [int(d[0].shape[0]) for d in a], [int(d[0].shape[0]) for d in b8]
            agree = [t for t in range(len(a)) if ca[t] == cb[t] and ca[t] > 0]
            diff = [max(float((a[t][i].float() - b8[t][i].float()).abs().max()) for t in agree) if agree else float('nan') for i in (0, 2, 3)]
            box = max(float((a[t][0][:, :4] - b8[t][0][:, :4]).abs().max()) for t in agree) if agree else float('nan')
            score = max(float((a[t][0][:, 4] - b8[t][0][:, 4]).abs().max()) for t in agree) if agree else float('nan')
            # rank by rank a swap of two near-equal scores shows as a large difference: also every batch-1 detection against the
            # NEAREST batch-8 box of its tile (largest coordinate difference), and the scores of those pairs
            near, near_score = [], []
            for t in agree:
                d = (a[t][0][:, None, :4] - b8[t][0][None, :, :4]).abs().amax(2)
                v, j = d.min(1)
                near.append(v), near_score.append((a[t][0][:, 4] - b8[t][0][j, 4]).abs())
            if not agree:
                raise SystemExit(f'no tile with equal detection counts: batch 1 {ca}, batch 8 {cb}')
            near, near_score = torch.cat(near), torch.cat(near_score)
            lines += ['# batch 8 against batch 1 on the 4096^2 scene, tile_detections:',
                      f'detections per tile: batch 1 {ca}', f'detections per tile: batch 8 {cb}',
                      f'tiles with equal counts: {len(agree)} of {len(a)}; rank by rank, max |difference| there: boxes {box:.4g} px, scores '
                      f'{score:.3g}, mask logits {diff[1]:.4g}, offsets {diff[2]:.4g} px',
                      f'nearest box of the same tile: within 0.5 px for {float((near < 0.5).float().mean()) * 100:.1f} % of the detections, '
                      f'median {float(near.median()):.3g} px, max {float(near.max()):.4g} px; |score difference| of those pairs: median '
                      f'{float(near_score.median()):.3g}, max {float(near_score.max()):.3g}']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
