#!/usr/bin/env python
"""What RandomRotate costs in data.to_device_batch: HIP-event time of the call for a batch of 8 x 1024^2 polygon samples (80
instances each, pinned staging as in the prefetching loader), every sample rotated by 90 degrees against none rotated -- the
unrotated batch takes the torch chain a batch took before the transform existed, and is the baseline.

    python tools/measure_rotate.py [--out profiles/rotate_measured.txt] [--reps 20]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    from bonai_amd import kernels as K
    from bonai_amd.data import parse_bonai_annotations, rotate_sample, to_device_batch
    from bonai_amd.synth import synth_bonai_anns
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    bs, size, n_inst = 8, 1024, 80
    rng = np.random.RandomState(0)
    staged = torch.from_numpy(rng.randint(0, 256, (bs, size, size, 3)).astype(np.uint8)).pin_memory()
    plain = []
    for i in range(bs):
        ann = parse_bonai_annotations(dict(width=size, height=size, filename=f't{i}.png'), synth_bonai_anns(seed=i, n=n_inst, size=size))
        plain.append(dict(img=staged[i].numpy(), img_rgb=True, gt_bboxes=ann['bboxes'], gt_labels=ann['labels'], gt_offsets=ann['offsets'],
                          gt_polygons=ann['masks'], gt_polygons_packed=K.pack_polygons(ann['masks'])))
    rotated = [rotate_sample(s, 90, defer_image=True) for s in plain]
    image_only = [{k: v for k, v in s.items() if k != 'mask_flips'} for s in rotated]
    n_masks = sum(len(s['gt_polygons']) for s in plain)
    cases = [('none rotated (torch chain; the baseline)', plain), ('all rotated by 90, image only (bitmaps left as rasterised)', image_only),
             ('all rotated by 90, image and bitmaps', rotated)]
    times = {name: [] for name, _ in cases}
    for rep in range(args.warmup + args.reps):                   # the cases alternate inside every repetition
        for name, samples in cases:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            batch = to_device_batch(samples, staged=staged)
            end.record()
            end.synchronize()
            if rep >= args.warmup:
                times[name].append(start.elapsed_time(end))
            del batch
    lines = [f'# data.to_device_batch, HIP-event time of one call: {bs} x {size}^2 polygon samples from pinned staging, {n_masks} instance',
             f'# bitmaps in the batch; median / min / max of {args.reps} calls after {args.warmup} warm-up, the cases alternating, one process,',
             '# one session; includes the 25 MB upload, Normalize, the rasterisation (loft_poly2mask) and the small-array copy',
             f'# device {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]})']
    base = float(np.median(times[cases[0][0]]))
    for name, _ in cases:
        t = np.array(times[name])
        lines.append(f'{name:62s} {np.median(t):8.3f} ms  (min {t.min():.3f}, max {t.max():.3f})  {np.median(t) - base:+.3f} ms against the baseline')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
