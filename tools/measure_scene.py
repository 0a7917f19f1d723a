#!/usr/bin/env python
"""Writes profiles/scene_measured.txt: what whole-scene inference (bonai_amd/scene.py) costs on top of its tiles.

    python tools/measure_scene.py [--out profiles/scene_measured.txt] [--step NAME]

Merge stage -- from the tiles' detections (scene-frame boxes, 28 x 28 logits, tile index, scores) to ``keep``:
  * fused    = kernels.scene_pair_counts + kernels.scene_suppress (csrc/scene.hip)
  * baseline = what the existing ops allow: candidate pairs from the integer windows in torch, kernels.mask_paste of both sides of every
               pair onto the pair's intersection crop (boxes moved to the crop's frame, crops padded to the largest one, ONE launch
               per side for all pairs -- far kinder to it than a launch per pair), ``&`` and sum, areas the same way, then the greedy
               loop on the host.  Moving a box moves the rounding of the paste's grid coordinate, so single boundary pixels can
               differ from the fused counts: the number of detections whose ``keep`` differs is reported, not asserted (exactness
               is the tests' subject, against whole-canvas bitmaps).
  scenes 2048^2 and 4096^2, tile 1024, overlap 256; synthetic buildings (8..78 px) at about 100 and about 1000 per tile, every
  building detected by each tile it lies in (clipped to the tile, jittered), smooth-blob logits plus noise.
Whole scene -- SceneDetector.run on a 4096^2 synthetic scene with the seeded synthetic weights (25 tiles): ms and peak device memory,
next to 25 x the single-tile time of simple_test with rle_masks='fused' on a 1024^2 tile (the method of tools/measure_tta.py).
Both paths of a comparison alternate in one process; medians of synchronised wall-clock runs after warm-up.  Without ``--step``
every step runs in a child process of its own under a time limit of its own, and the run stops at the first step that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE, OVERLAP, S = 1024, 256, 28
STEPS = [('merge 2048 ~100/tile', 2048, 100, 150), ('merge 2048 ~1000/tile', 2048, 1000, 240), ('merge 4096 ~100/tile', 4096, 100, 200),
         ('merge 4096 ~1000/tile', 4096, 1000, 360), ('scene 4096', 4096, 0, 360)]          # name, scene side, per tile, time limit (s)


def timed_pair(a, b, reps, warm=1):
    for _ in range(warm):
        a()
        b()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((a, ta), (b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ta), statistics.median(tb)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def synthetic_detections(side, per_tile, seed=0):
    """-> (scene boxes [N,4], tile boxes [N,4], tiles [N], scores [N], logits [N,S,S], origins [T,2]) on the device."""
    from bonai_amd.scene import tile_grid
    origins = tile_grid(side, side, TILE, OVERLAP)
    rng = np.random.RandomState(seed)
    nb = int(per_tile * len(origins) * 0.62)          # a building lies in about 1 / 0.62 tiles at this overlap
    xy = rng.uniform(0, side - 80, (nb, 2))
    b = np.concatenate([xy, xy + 8 + rng.uniform(0, 70, (nb, 2))], 1)
    sb, tb, ti = [], [], []
    for t, (x0, y0) in enumerate(origins.tolist()):
        inside = (b[:, 2] > x0 + 4) & (b[:, 0] < x0 + TILE - 4) & (b[:, 3] > y0 + 4) & (b[:, 1] < y0 + TILE - 4)
        loc = b[inside] - [x0, y0, x0, y0] + rng.uniform(-1, 1, (int(inside.sum()), 4))
        loc = np.clip(loc, 0, TILE)
        tb.append(loc), sb.append(loc + [x0, y0, x0, y0]), ti.append(np.full(len(loc), t, np.int32))
    sb, tb, ti = np.concatenate(sb).astype(np.float32), np.concatenate(tb).astype(np.float32), np.concatenate(ti)
    N = len(sb)
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing='ij')
    blob = 4 - 8 * ((yy - 13.5) ** 2 + (xx - 13.5) ** 2) / 14 ** 2
    logits = (blob + torch.randn(N, S, S, generator=g)).cuda()
    scores = torch.rand(N, generator=g).cuda()
    return torch.from_numpy(sb).cuda(), torch.from_numpy(tb).cuda(), torch.from_numpy(ti).cuda(), scores, logits, torch.from_numpy(origins).cuda()


def windows(boxes, side):
    x0 = (boxes[:, 0].floor() - 1).clamp(0, side)
    x1 = (boxes[:, 2].ceil() + 1).clamp(0, side)
    y0 = (boxes[:, 1].floor() - 1).clamp(0, side)
    y1 = (boxes[:, 3].ceil() + 1).clamp(0, side)
    return torch.stack([x0, x1, y0, y1], 1)


def baseline_merge(boxes, tiles, scores, trunc, logits, side, merge_thr):
    from bonai_amd import kernels as K
    N = boxes.shape[0]
    win = windows(boxes, side)
    pi, pj = [], []
    for r0 in range(0, N, 4096):                     # candidate pairs, a block of rows at a time
        a = win[r0:r0 + 4096, None]
        meet = (torch.maximum(a[..., 0], win[None, :, 0]) < torch.minimum(a[..., 1], win[None, :, 1])) & \
               (torch.maximum(a[..., 2], win[None, :, 2]) < torch.minimum(a[..., 3], win[None, :, 3])) & \
               (tiles[r0:r0 + 4096, None] != tiles[None]) & (torch.arange(r0, min(r0 + 4096, N), device=boxes.device)[:, None] <
                                                               torch.arange(N, device=boxes.device)[None])
        ij = meet.nonzero()
        pi.append(ij[:, 0] + r0), pj.append(ij[:, 1])
    pi, pj = torch.cat(pi), torch.cat(pj)

    def crop_counts(idx_a, idx_b, cw):               # |mask_a & mask_b| on the crops cw = (x0, x1, y0, y1)
        w, h = int((cw[:, 1] - cw[:, 0]).max()), int((cw[:, 3] - cw[:, 2]).max())
        valid = (torch.arange(w, device=cw.device)[None, None] < (cw[:, 1] - cw[:, 0])[:, None, None]) & \
                (torch.arange(h, device=cw.device)[None, :, None] < (cw[:, 3] - cw[:, 2])[:, None, None])
        shift = torch.stack([cw[:, 0], cw[:, 2], cw[:, 0], cw[:, 2]], 1)
        out = valid
        for idx in (idx_a, idx_b):
            if idx is not None:
                out = out & K.mask_paste(logits[idx], boxes[idx] - shift, h, w, 0.5).bool()
        return out.flatten(1).sum(1)
    area = crop_counts(torch.arange(N, device=boxes.device), None, win)
    inter = torch.zeros(0, dtype=torch.int64, device=boxes.device)
    if pi.numel():
        a, b = win[pi], win[pj]
        cw = torch.stack([torch.maximum(a[:, 0], b[:, 0]), torch.minimum(a[:, 1], b[:, 1]), torch.maximum(a[:, 2], b[:, 2]),
                          torch.minimum(a[:, 3], b[:, 3])], 1)
        inter = torch.cat([crop_counts(pi[c:c + 8192], pj[c:c + 8192], cw[c:c + 8192]) for c in range(0, pi.numel(), 8192)])
    area, inter, pi, pj = area.cpu().numpy(), inter.cpu().numpy(), pi.cpu().numpy(), pj.cpu().numpy()
    sc, tr = scores.cpu().numpy(), trunc.cpu().numpy()
    nbr = [[] for _ in range(N)]
    edge = (np.minimum(area[pi], area[pj]) > 0) & (inter > merge_thr * np.minimum(area[pi], area[pj]))
    for i, j in zip(pi[edge].tolist(), pj[edge].tolist()):
        nbr[i].append(j)
        nbr[j].append(i)
    keep, seen = np.zeros(N, bool), np.zeros(N, bool)
    for n in sorted(range(N), key=lambda n: (bool(tr[n]), -float(sc[n]), n)):
        keep[n] = not any(seen[m] and keep[m] for m in nbr[n])
        seen[n] = True
    return keep, len(pi)


def merge_step(name, side, per_tile):
    from bonai_amd import kernels as K
    from bonai_amd.scene import SceneDetector
    boxes, tboxes, tiles, scores, logits, origins = synthetic_detections(side, per_tile)
    N = boxes.shape[0]

    class _Rule(SceneDetector):                      # the truncation rule without a model
        def __init__(self):
            self.tile, self.border = (TILE, TILE), 2
    trunc = _Rule().truncated(tboxes, tiles, origins, side, side)
    out = {}

    def fused():
        area, recs = K.scene_pair_counts(logits, boxes, tiles, side, side, 0.5)
        out['fused'] = K.scene_suppress(recs, area, scores, trunc, 0.5).bool().cpu().numpy()
        out['records'] = int(recs.shape[0])

    def baseline():
        out['base'], out['pairs'] = baseline_merge(boxes, tiles, scores, trunc, logits, side, 0.5)
    reps = 5 if N < 5000 else 3
    tb, tf = timed_pair(baseline, fused, reps)
    return dict(name=name, N=N, tiles=int(origins.shape[0]), pairs=out['records'], kept=int(out['fused'].sum()),
                differ=int((out['fused'] != out['base']).sum()), base_ms=tb, fused_ms=tf, base_mib=peak_mib(baseline),
                fused_mib=peak_mib(fused))


def scene_step(name, side):
    from bonai_amd import kernels as K
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from bonai_amd.scene import SceneDetector, tile_grid
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(1)
    scene = (torch.randn(side, side, 3, generator=g) * 58 + 120).clamp(0, 255).to(torch.uint8).cuda()
    det = SceneDetector(m, tile=TILE, overlap=OVERLAP)
    T = len(tile_grid(side, side, TILE, OVERLAP))
    img = K.image_prep_d4(scene[:TILE, :TILE][None].contiguous(), [0], [False], det.mean, det.std)
    meta = [dict(img_shape=(TILE, TILE, 3), pad_shape=(TILE, TILE, 3), ori_shape=(TILE, TILE, 3), scale_factor=np.ones(4, np.float32),
                 flip=False)]
    rcnn = m.roi_head.test_cfg
    out = {}

    def one_tile():
        rcnn['rle_masks'] = 'fused'
        try:
            with torch.no_grad():
                out['tile'] = m(img=[img], img_metas=[meta], return_loss=False, rescale=True)
        finally:
            rcnn.pop('rle_masks')

    def whole():
        out['scene'] = det.run(scene)
    t_tile, t_scene = timed_pair(one_tile, whole, 3)
    n_tile = sum(len(d[0]) for d in det.tile_detections(scene)[1])
    return dict(name=name, tiles=T, tile_ms=t_tile, scene_ms=t_scene, scene_mib=peak_mib(whole), tile_mib=peak_mib(one_tile),
                tile_dets=int(out['tile'][0][0].shape[0]), all_dets=int(n_tile), kept=len(out['scene']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_measured.txt'))
    ap.add_argument('--step', help='run one step in this process and print its JSON line')
    args = ap.parse_args()
    if args.step:
        name, side, per_tile, _ = next(s for s in STEPS if s[0] == args.step)
        print('RESULT ' + json.dumps(merge_step(name, side, per_tile) if per_tile else scene_step(name, side)), flush=True)
        return
    from bonai_amd import build
    rows = []
    for name, _, _, limit in STEPS:                  # a fresh process per step: a step that faults or hangs ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name], capture_output=True, text=True, timeout=limit)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not line:
            raise SystemExit(f'step {name!r} failed with exit status {p.returncode}: {p.stderr[-2000:]}')
        rows.append(json.loads(line[0][7:]))
        print(rows[-1], flush=True)
    dev = subprocess.run([sys.executable, '-c', 'import torch; print(torch.cuda.get_device_name(0))'], capture_output=True, text=True,
                         timeout=120).stdout.strip()
    merge, scene = [r for r in rows if 'base_ms' in r], [r for r in rows if 'scene_ms' in r]
    lines = [f'# tools/measure_scene.py, source hash {build.source_hash()}, {dev}, one session',
             f'# merge stage, tile {TILE}, overlap {OVERLAP}: scene-frame boxes + fp32 logits [N,28,28] + tile index + scores -> keep [N] on the host',
             '# fused = scene_pair_counts + scene_suppress (csrc/scene.hip); baseline = windows in torch, mask_paste of both sides of every',
             '# candidate pair on its intersection crop (one launch per side and 8192 pairs), & and sum, greedy loop on the host;',
             '# median of alternating synchronised wall-clock runs after 1 warm-up run (5 runs, 3 at N >= 5000), ms; peak =',
             '# torch.cuda.max_memory_allocated of the stage alone, MiB (inputs included); differ = detections whose keep differs',
             '# (the baseline pastes in the crop\'s frame: boundary pixels can round differently)',
             '# case                     N | tiles | records | kept | baseline ms | fused ms | ratio | baseline MiB | fused MiB | differ']
    for r in merge:
        lines.append(f'{r["name"]:22s} {r["N"]:6d} | {r["tiles"]:5d} | {r["pairs"]:7d} | {r["kept"]:4d} | {r["base_ms"]:11.2f} | '
                     f'{r["fused_ms"]:8.2f} | x{r["base_ms"] / r["fused_ms"]:<5.1f}| {r["base_mib"]:12.1f} | {r["fused_mib"]:9.1f} | {r["differ"]}')
    lost = [r['name'] for r in merge if r['fused_ms'] > r['base_ms']]
    small = merge[0]
    lines.append('condition (the fused stage does not lose at the smallest load, ' + small['name'] + '): ' +
                 ('holds' if small['fused_ms'] <= small['base_ms'] else 'FAILS') + ('' if not lost else f'; slower for {lost}'))
    for r in scene:
        lines += [f'# whole scene: SceneDetector.run on a {r["name"].split()[1]}^2 random uint8 scene, synthetic weights, {r["tiles"]} tiles; one tile =',
                  "# simple_test with rle_masks='fused' on a 1024^2 tile of it, prepared tile given (synthetic weights: detection counts",
                  '# say nothing about trained ones); 3 alternating runs after 1 warm-up, median ms',
                  f'run() {r["scene_ms"]:.1f} ms, peak {r["scene_mib"]:.0f} MiB | one tile {r["tile_ms"]:.1f} ms, peak {r["tile_mib"]:.0f} MiB | '
                  f'{r["tiles"]} x one tile = {r["tiles"] * r["tile_ms"]:.1f} ms | tiling + merging add {r["scene_ms"] - r["tiles"] * r["tile_ms"]:.1f} ms '
                  f'| detections: {r["all_dets"]} over the tiles, {r["kept"]} kept ({r["tile_dets"]} on the one tile)']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
