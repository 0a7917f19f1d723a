#!/usr/bin/env python
"""What Resize costs on the device.  Two comparisons, HIP-event times, every case alternating inside one process:

1. kernels.image_resize_prep on 8 x 1024^2 uint8 tiles -> 8 x {768^2, 1024^2, 1280^2} against a chain of torch ops of the same
   geometry (uint8 -> float, F.interpolate(bilinear), flip, normalise, pad), with the achieved bytes/s over the algorithmic bytes
   (source read once, output written once); and kernels.mask_resize_u8 on 591 bitmaps of 1024^2 against F.interpolate(nearest).
2. data.to_device_batch on the polygon batch of tools/measure_rotate.py: the plain path (no ``resize``: what the loader did before
   Resize existed) against the identity-scale ``resize`` path, with the run-to-run spread of the plain path next to it.

    python tools/measure_resize.py [--out profiles/resize_measured.txt] [--reps 20]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    del out
    return start.elapsed_time(end)


def torch_chain(u8, side, pad):
    x = torch.nn.functional.interpolate(u8.permute(0, 3, 1, 2).float(), size=(side, side), mode='bilinear', align_corners=False)
    x = x.flip(1).flip(3)                                                                  # to_rgb, horizontal RandomFlip
    x = (x - torch.tensor(MEAN, device=u8.device).view(1, 3, 1, 1)) / torch.tensor(STD, device=u8.device).view(1, 3, 1, 1)
    return torch.nn.functional.pad(x, (0, pad - side, 0, pad - side))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    from bonai_amd import kernels as K
    from bonai_amd.data import parse_bonai_annotations, resize_sample, to_device_batch
    from bonai_amd.synth import synth_bonai_anns
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    bs, size, n_inst = 8, 1024, 80
    rng = np.random.RandomState(0)
    staged = torch.from_numpy(rng.randint(0, 256, (bs, size, size, 3)).astype(np.uint8)).pin_memory()
    u8 = staged.cuda()
    masks = (torch.rand(591, size, size, device='cuda') < 0.3).to(torch.uint8)
    med = lambda v: float(np.median(v))                                                    # noqa: E731
    lines = [f'# device {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}); HIP-event times, '
             f'median / min / max of {args.reps} calls after {args.warmup} warm-up, the cases alternating, one process, one session',
             f'# 1. kernel against a torch-op chain of the same geometry, {bs} x {size}^2 uint8 tiles, element MIRROR_X, canvas = target']
    for side in (768, 1024, 1280):
        pad = -(-side // 64) * 64
        cases = [('loft_image_resize_prep_d4', lambda: K.image_resize_prep(u8, (side, side), (pad, pad), [K.D4_MIRROR_X] * bs, [False] * bs, MEAN, STD)),
                 ('torch chain', lambda: torch_chain(u8, side, pad))]
        t = {n: [] for n, _ in cases}
        for rep in range(args.warmup + args.reps):
            for n, fn in cases:
                ms = timed(fn)
                if rep >= args.warmup:
                    t[n].append(ms)
        nbytes = bs * (size * size * 3 + 3 * pad * pad * 4)
        for n, _ in cases:
            v = np.array(t[n])
            extra = f'  {nbytes / (med(v) * 1e-3) / 1e9:7.1f} GB/s over {nbytes / 1e6:.1f} MB (source once, output once)' if n.startswith('loft') else ''
            lines.append(f'{size}^2 -> {side}^2  {n:28s} {med(v):8.3f} ms  (min {v.min():.3f}, max {v.max():.3f}){extra}')
        lines.append(f'{size}^2 -> {side}^2  fused kernel / torch chain = {med(t[cases[0][0]]) / med(t[cases[1][0]]):.3f}')
    for side in (768, 1280):
        cases = [('loft_mask_resize_d4_u8', lambda: K.mask_resize_u8(masks, (side, side), (side, side), K.D4_MIRROR_X)),
                 ('F.interpolate(nearest) + flip', lambda: torch.nn.functional.interpolate(masks[None], size=(side, side), mode='nearest')[0].flip(2).contiguous())]
        t = {n: [] for n, _ in cases}
        for rep in range(args.warmup + args.reps):
            for n, fn in cases:
                ms = timed(fn)
                if rep >= args.warmup:
                    t[n].append(ms)
        nbytes = 591 * (size * size + side * side)
        for n, _ in cases:
            v = np.array(t[n])
            extra = f'  {nbytes / (med(v) * 1e-3) / 1e9:7.1f} GB/s over {nbytes / 1e6:.1f} MB' if n.startswith('loft') else ''
            lines.append(f'591 bitmaps {size}^2 -> {side}^2  {n:30s} {med(v):8.3f} ms  (min {v.min():.3f}, max {v.max():.3f}){extra}')
    del masks
    plain = []
    for i in range(bs):
        ann = parse_bonai_annotations(dict(width=size, height=size, filename=f't{i}.png'), synth_bonai_anns(seed=i, n=n_inst, size=size))
        plain.append(dict(img=staged[i].numpy(), img_rgb=True, gt_bboxes=ann['bboxes'], gt_labels=ann['labels'], gt_offsets=ann['offsets'],
                          gt_polygons=ann['masks'], gt_polygons_packed=K.pack_polygons(ann['masks'])))
    resized = [resize_sample(s, (size, size), True, 32) for s in plain]
    cases = [('plain path (no resize; the baseline)', plain), ('plain path again (its run-to-run spread)', plain),
             ('resize at the identity scale', resized)]
    t = {n: [] for n, _ in cases}
    for rep in range(args.warmup + args.reps):
        for n, samples in cases:
            ms = timed(lambda: to_device_batch(samples, staged=staged))
            if rep >= args.warmup:
                t[n].append(ms)
    lines.append(f'# 2. data.to_device_batch, one call: {bs} x {size}^2 polygon samples from pinned staging, {sum(len(s["gt_polygons"]) for s in plain)} bitmaps '
                 '(upload, Normalize, rasterisation, small-array copy)')
    base = med(t[cases[0][0]])
    for n, _ in cases:
        v = np.array(t[n])
        lines.append(f'{n:44s} {med(v):8.3f} ms  (min {v.min():.3f}, max {v.max():.3f})  {med(v) - base:+.3f} ms against the baseline')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
