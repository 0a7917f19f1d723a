#!/usr/bin/env python
"""Writes profiles/rle_measured.txt: the mask result stage of one 1024^2 tile -- from the class-selected mask logits and the boxes to
the list of COCO RLE dicts -- on the bitmap path (kernels.mask_paste + rle.rle_encode_masks) and on the fused one
(kernels.mask_paste_rle, csrc/mask_rle.hip), in one process, alternating.

    python tools/measure_rle.py [--out profiles/rle_measured.txt] [--step NAME]

  * N = 100, 1000, 2000 detections, boxes with the size distribution of tools/measure_tta.py (8..78 px, anywhere on the tile),
    logits of a smooth blob plus noise (building-like masks: a few runs per column)
  * V = 3 views (none / horizontal / vertical) at N = 100 against kernels.mask_paste_views + rle_encode_masks
  * the footprint variant at N = 100 against mask_paste + mask_translate + rle_encode_masks
  * torch.cuda.max_memory_allocated of each stage on its own (inputs included)
Every stage is checked for equal bytes before it is timed.  Without ``--step`` every step runs in a child process of its own under
a time limit of its own, and the run stops at the first step that fails.  Timing: warm-up, then the median of repeated synchronised
wall-clock runs of the whole stage (device work and the host's part of it; both paths end in host objects).
Expectation checked here: the fused stage is slower than the bitmap stage nowhere.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = [('N=100', 100, 1, False, 120), ('N=1000', 1000, 1, False, 240), ('N=2000', 2000, 1, False, 420),
         ('N=100 V=3', 100, 3, False, 120), ('N=100 footprint', 100, 1, True, 120)]      # name, N, V, footprint, time limit (s)


def timed_pair(a, b, reps, warm=2):
    """Median wall-clock ms of a and of b, alternating so that both see the same state of the machine."""
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


def step(name, size):
    from bonai_amd import kernels as K
    from bonai_amd.rle import rle_encode_masks
    _, N, V, footprint, _ = next(s for s in STEPS if s[0] == name)
    H = W = size
    S = 28
    g = torch.Generator().manual_seed(0)
    xy = torch.rand(N, 2, generator=g) * (H - 80)
    boxes = torch.cat([xy, xy + 8 + torch.rand(N, 2, generator=g) * 70], 1).cuda()
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing='ij')
    blob = 4 - 8 * ((yy - 13.5) ** 2 + (xx - 13.5) ** 2) / 14 ** 2
    logits = (blob + torch.randn(V, N, S, S, generator=g)).cuda()
    table = K.tta_view_table([0, 2, 4][:V], 'cuda')
    offs = ((torch.rand(N, 2, generator=g) * 60 - 30).cuda()) if footprint else None

    def bitmap():
        m = K.mask_paste(logits[0], boxes, H, W, 0.5) if V == 1 else K.mask_paste_views(logits, boxes, table, H, W, 0.5)
        if footprint:
            m = K.mask_translate(m, offs)
        return rle_encode_masks(m)

    def fused():
        return K.mask_paste_rle(logits[0] if V == 1 else logits, boxes, H, W, 0.5, views=table if V > 1 else None, offsets=offs)
    want, got = bitmap(), fused()
    if want != got:
        raise SystemExit(f'{name}: the fused strings differ from the bitmap path\'s')
    runs = sum(len(r['counts']) for r in got)
    tb, tf = timed_pair(bitmap, fused, reps=5 if N >= 1000 else 9)
    return dict(name=name, bitmap_ms=tb, fused_ms=tf, bitmap_mib=peak_mib(bitmap), fused_mib=peak_mib(fused), bytes=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rle_measured.txt'))
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--step', help='run one step in this process and print its JSON line')
    args = ap.parse_args()
    if args.step:
        print('RESULT ' + json.dumps(step(args.step, args.size)), flush=True)
        return
    from bonai_amd import build
    rows = []
    for name, _, _, _, limit in STEPS:           # a fresh process per step: a step that faults or hangs ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name, '--size', str(args.size)], capture_output=True,
                           text=True, timeout=limit)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not line:
            raise SystemExit(f'step {name!r} failed with exit status {p.returncode}: {p.stderr[-2000:]}')
        rows.append(json.loads(line[0][7:]))
        print(rows[-1], flush=True)
    dev = subprocess.run([sys.executable, '-c', 'import torch; print(torch.cuda.get_device_name(0))'], capture_output=True, text=True,
                         timeout=120).stdout.strip()
    lines = [f'# tools/measure_rle.py, source hash {build.source_hash()}, {dev}, one session',
             f'# result stage of one {args.size}^2 tile: class-selected fp32 mask logits [V,N,28,28] + boxes -> N COCO RLE dicts on the host',
             '# bitmap = mask_paste(_views) [+ mask_translate] + rle.rle_encode_masks; fused = mask_paste_rle (csrc/mask_rle.hip); equal bytes',
             '# checked first; median of alternating synchronised wall-clock runs after 2 warm-up runs (9 runs, 5 at N >= 1000), ms;',
             '# peak = torch.cuda.max_memory_allocated of the stage alone, MiB (inputs included)',
             '# case              bitmap ms | fused ms | ratio | bitmap peak MiB | fused peak MiB | string bytes']
    slower = []
    for r in rows:
        lines.append(f'{r["name"]:18s} {r["bitmap_ms"]:10.2f} | {r["fused_ms"]:8.2f} | x{r["bitmap_ms"] / r["fused_ms"]:<6.1f}| '
                     f'{r["bitmap_mib"]:15.1f} | {r["fused_mib"]:14.1f} | {r["bytes"]}')
        if r['fused_ms'] > r['bitmap_ms']:
            slower.append(r['name'])
    lines.append('expectation (the fused stage is slower than the bitmap stage nowhere): ' + ('holds' if not slower else f'FAILS for {slower}'))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    if slower:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
