#!/usr/bin/env python
"""What COCO AP costs (bonai_amd/coco_eval.py): the matching of COCOeval.evaluateImg and the accumulation of
COCOeval.accumulate for 64 synthetic tiles at two loads -- 100 detections x 80 ground truths and 1000 x 300 per tile -- on the
device (kernels.coco_match, 8 tiles per launch as CocoEvaluator queues them, + the read-back of the bit words;
kernels.coco_accumulate + the read-back of precision / recall) against the numpy restatement of the published cocoapi source
(tests/coco_eval_restatement.py), alternating in one process.  The restatement's evaluateImg is a triple Python loop: it is
timed on ``--host-tiles`` tiles per load and the 64-tile figure is that time scaled, and marked as such.  Where both ran, the
results are checked to be identical.  The segm IoU part (kernels.mask_pair_counts + kernels.coco_mask_iou on 1024^2 bitmaps
against the restatement's pixel counting, the latter on a sample of pairs and scaled) is reported separately.

Host wall time of work that ends in a device synchronise, median / min / max.

    python tools/measure_coco.py [--out profiles/coco_measured.txt] [--reps 7] [--host-tiles 4,1]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import coco_eval_restatement as R  # noqa: E402

TILES, SIZE, MAX_DETS = 64, 1024, (100, 300, 1000)


def _timed(fn, sync=True):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ts):
    t = np.asarray(ts)
    return f'{np.median(t):10.3f} ms  (min {t.min():.3f}, max {t.max():.3f}, n={t.size})'


def _tile(rng, D, G):
    """xywh ground truths of 16..120 px sides, detections = jittered ground truths and strays, float32 scores in descending order."""
    gt = np.concatenate([rng.uniform(0, SIZE - 130, (G, 2)), rng.uniform(16, 120, (G, 2))], 1)
    dt = gt[rng.randint(0, G, D)] + rng.normal(0, 4, (D, 4))
    stray = rng.uniform(size=D) < 0.3
    dt[stray] = np.concatenate([rng.uniform(0, SIZE - 130, (D, 2)), rng.uniform(16, 120, (D, 2))], 1)[stray]
    dt[:, 2:] = np.maximum(dt[:, 2:], 2)
    scores = np.sort(rng.uniform(0.05, 1, D).astype(np.float32))[::-1].copy()
    return dict(dt=dt, gt=gt, crowd=(rng.uniform(size=G) < 0.03).astype(np.uint8), scores=scores, det_area=dt[:, 2] * dt[:, 3],
                gt_area=gt[:, 2] * gt[:, 3])


def load(D, G, reps, host_tiles, lines):
    from bonai_amd import kernels as K
    rng = np.random.RandomState(D)
    tiles = [_tile(rng, D, G) for _ in range(TILES)]
    thrs, rec = R.default_iou_thrs(), R.default_rec_thrs()
    T = len(thrs)
    ious = [K.coco_box_iou(t['dt'], t['gt'], t['crowd']) for t in tiles]
    cat = lambda k, ts: np.concatenate([t[k] for t in ts])

    def match_device():
        out = []
        for b in range(0, TILES, 8):
            ts = tiles[b:b + 8]
            _, bits, npig = K.coco_match(ious[b:b + 8], [D] * len(ts), [G] * len(ts), cat('det_area', ts), cat('gt_area', ts), cat('crowd', ts),
                                         thrs)
            out.append((bits.cpu().numpy(), npig.cpu().numpy()))
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    bits, npig = match_device()
    scores, rank = cat('scores', tiles), np.tile(np.arange(D, dtype=np.int32), TILES)

    def acc_device():
        p, r = K.coco_accumulate(scores, bits, rank, npig.sum(0), MAX_DETS, rec, T)
        return p.cpu().numpy(), r.cpu().numpy()

    def match_host(n):
        host = [x.cpu().numpy() for x in ious[:n]]
        return [[R.evaluate_img(host[i], t['det_area'], t['gt_area'], t['crowd'], rng_, thrs) for rng_ in R.AREA_RNG]
                for i, t in enumerate(tiles[:n])]
    words = bits.view(np.uint64)
    flag = lambda w, a: np.stack([(w >> np.uint64(a * T + t)) & np.uint64(1) for t in range(T)]).astype(bool)
    E = [[dict(scores=t['scores'], dtm=np.where(flag(words[i * D:(i + 1) * D, 0], a), 0, -1), dt_ig=flag(words[i * D:(i + 1) * D, 1], a),
               npig=int(npig[i, a])) for i, t in enumerate(tiles)] for a in range(4)]

    def acc_host():
        res = [R.accumulate(E[a], MAX_DETS, rec, T) for a in range(4)]
        return np.stack([x[0] for x in res], 2), np.stack([x[1] for x in res], 1)
    times = {k: [] for k in ('match_device', 'acc_device', 'match_host', 'acc_host')}
    for rep in range(1 + reps):
        for name, fn in (('match_device', match_device), ('acc_device', acc_device)):
            t, _ = _timed(fn)
            if rep:
                times[name].append(t)
        if rep < 2:                                                    # (seconds per call: twice, between the device calls)
            t, evs = _timed(lambda: match_host(host_tiles), sync=False)
            times['match_host'].append(t)
            t, (hp, hr) = _timed(acc_host, sync=False)
            times['acc_host'].append(t)
    for i, per_area in enumerate(evs):                                 # identical where both ran
        for a, ev in enumerate(per_area):
            assert np.array_equal(flag(words[i * D:(i + 1) * D, 0], a), ev['dtm'] >= 0) and np.array_equal(flag(words[i * D:(i + 1) * D, 1], a), ev['dt_ig'])
            assert npig[i, a] == ev['npig']
    dp, dr = acc_device()
    assert np.array_equal(dp.view(np.int64), hp.view(np.int64)) and np.array_equal(dr.view(np.int64), hr.view(np.int64))
    mh = np.asarray(times['match_host']) * (TILES / host_tiles)
    lines.append(f'{TILES} tiles, {D} detections x {G} ground truths each, T = {T} thresholds, 4 area ranges (results identical, checked):')
    lines.append(f"  {'matching, device (8 launches + read-backs)':58s} {_stats(times['match_device'])}")
    lines.append(f"  {f'matching, numpy restatement ({host_tiles} tiles timed, x {TILES // host_tiles})':58s} {_stats(mh)}")
    lines.append(f"  {'accumulation, device (sort + 1 launch + read-back)':58s} {_stats(times['acc_device'])}")
    lines.append(f"  {'accumulation, numpy restatement':58s} {_stats(times['acc_host'])}")
    return np.median(times['match_device']) + np.median(times['acc_device']), np.median(mh) + np.median(times['acc_host'])


def segm_iou(D, G, reps, pairs, lines):
    from bonai_amd import kernels as K
    rng = np.random.RandomState(7 + D)
    t = _tile(rng, D, G)
    rect = lambda b: [[float(v) for v in (b[0], b[1], b[0] + b[2], b[1], b[0] + b[2], b[1] + b[3], b[0], b[1] + b[3])]]
    pm, gm = K.poly2mask([rect(b) for b in t['dt']], SIZE, SIZE), K.poly2mask([rect(b) for b in t['gt']], SIZE, SIZE)
    win = np.stack([np.floor(t['dt'][:, 0]) - 2, np.floor(t['dt'][:, 1]) - 2, np.ceil(t['dt'][:, 0] + t['dt'][:, 2]) + 2,
                    np.ceil(t['dt'][:, 1] + t['dt'][:, 3]) + 2], 1)

    def device():
        inter, ap, ag = K.mask_pair_counts(pm, gm, win)
        return K.coco_mask_iou(inter, ap, ag, t['crowd']).cpu().numpy()
    nd = max(1, pairs // G)
    hp, hg = pm[:nd].cpu().numpy() != 0, gm.cpu().numpy() != 0
    times = {'device': [], 'host': []}
    for rep in range(1 + reps):
        tm, got = _timed(device)
        if rep:
            times['device'].append(tm)
        if rep < 2:
            tm, want = _timed(lambda: R.mask_iou(hp, hg, t['crowd']), sync=False)
            times['host'].append(tm)
    assert np.array_equal(got[:nd].view(np.int64), want.view(np.int64))
    lines.append(f'segm IoU of one {SIZE}^2 tile, {D} x {G} bitmaps (results identical on the pairs both computed, checked):')
    lines.append(f"  {'mask_pair_counts + coco_mask_iou + read-back':58s} {_stats(times['device'])}")
    lines.append(f"  {f'numpy restatement ({nd * G} pairs timed, x {D / nd:.0f})':58s} {_stats(np.asarray(times['host']) * (D / nd))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-tiles', default='4,1', help='tiles the numpy matching is timed on, per load')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    host_tiles = [int(v) for v in args.host_tiles.split(',')]
    lines = ['# COCO AP: matching + accumulation, device path against the numpy restatement of cocoapi (tests/coco_eval_restatement.py);',
             f'# host wall time of work ending in a device synchronise, median (min, max) of {args.reps} calls after 1 warm-up, the cases',
             '# alternating in one process; the restatement is timed twice, its matching on a few tiles and scaled (marked)',
             f'# device {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]})']
    for (D, G), n in zip(((100, 80), (1000, 300)), host_tiles):
        dev, host = load(D, G, args.reps, n, lines)
        lines.append(f'  matching + accumulation: device {dev:.3f} ms, numpy {host:.1f} ms')
    for (D, G), pairs in (((100, 80), 400), ((1000, 300), 600)):
        segm_iou(D, G, args.reps, pairs, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
