#!/usr/bin/env python
"""Writes profiles/tta_measured.txt: test-time augmentation on one 1024^2 tile in bf16 (synthetic weights).

    python tools/measure_tta.py [--out profiles/tta_measured.txt]

  * time per image of simple_test, and of aug_test with V = 3 (none / horizontal / vertical) and V = 8 (all symmetries)
  * the merge stages at V = 3, n = 1000 RoIs / 100 detections, each against a plain torch-op composition of the same arithmetic: the
    per-view loop of the reference's aug_test_* (bbox_mapping, softmax, decode, map back, stack, mean) and, for the masks, the host
    round trip aug_test_mask makes (sigmoid().cpu().numpy(), np.mean, back to the device, paste).  That composition is the baseline,
    not the code under test.  Expectation checked here: no fused merge is slower than its baseline.
Timing: warm-up, then the median of repeated synchronised wall-clock runs of the whole stage (the stages are chains of short launches
and host work; a device-event interval would leave the host part out).
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


def timed(fn, reps=15, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tta_measured.txt'))
    ap.add_argument('--size', type=int, default=1024)
    args = ap.parse_args()
    from bonai_amd import build, kernels as K, tta
    from bonai_amd.config import Config
    from bonai_amd.data import d4_apply
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    from oracle.synth_weights import synth_tensor
    lines = [f'# tools/measure_tta.py, source hash {build.source_hash()}, {torch.cuda.get_device_name(0)}, one session',
             f'# one {args.size}^2 tile, bf16, synthetic weights; median of 15 synchronised wall-clock runs after 3 warm-up runs, ms']
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    m = m.cuda().eval()
    data = make_batch(1, args.size, 40, device='cuda')
    img = data['img'].cpu().numpy()
    for name, views in (('simple_test', [None]), ('aug_test V=3', [None, 'horizontal', 'vertical']),
                        ('aug_test V=8', [None, 'horizontal', 'vertical', 90, 180, 270])):
        if name.endswith('V=8'):
            elems = [0, 2, 4, 3, 6, 5, 1, 7]
            metas = [[dict(tta.view_meta(data['img_metas'][0], None), **{tta.META_KEY: e})] for e in elems]
        else:
            elems = [tta.view_element(v) for v in views]
            metas = [[tta.view_meta(data['img_metas'][0], v)] for v in views]
        imgs = [torch.from_numpy(np.ascontiguousarray(d4_apply(img, e, axes=(2, 3)))).cuda() for e in elems]

        def run():
            with torch.no_grad():
                return m(img=imgs, img_metas=metas, return_loss=False, rescale=True)
        n = run()[0][0].shape[0]
        lines.append(f'{name:14s} {timed(run, reps=7, warm=2):9.2f} ms per image   ({n} detections)')

    # ---- merge stages against the torch-op per-view loop
    V, H, W, n, nd, S = 3, args.size, args.size, 1000, 100, 28
    elems = [0, 2, 4]
    dirs = [None, 'horizontal', 'vertical']
    table = K.tta_view_table(elems, 'cuda')
    g = torch.Generator().manual_seed(0)
    xy = torch.rand(n, 2, generator=g) * (H - 80)
    boxes = torch.cat([xy, xy + 8 + torch.rand(n, 2, generator=g) * 70], 1).cuda()
    means, stds = (0., 0., 0., 0.), (.1, .1, .2, .2)

    def flip(b, d):
        if d is None:
            return b
        o = b.clone()
        if d == 'horizontal':
            o[:, 0::4], o[:, 2::4] = W - b[:, 2::4], W - b[:, 0::4]
        else:
            o[:, 1::4], o[:, 3::4] = H - b[:, 3::4], H - b[:, 1::4]
        return o
    rois = K.tta_view_rois(boxes, table, V, H, W)
    bp, cs = torch.randn(V * n, 4, device='cuda'), torch.randn(V * n, 2, device='cuda')

    def base_rois():
        return torch.cat([torch.cat([b.new_full((n, 1), v), b], 1) for v, b in enumerate(flip(boxes, d) for d in dirs)], 0)

    def base_bboxes():
        bs, ss = [], []
        for v, d in enumerate(dirs):
            sl = slice(v * n, (v + 1) * n)
            ss.append(torch.softmax(cs[sl], 1))
            bs.append(flip(K.delta2bbox(rois[sl, 1:], bp[sl], means, stds, (H, W)), d))
        return torch.stack(bs).mean(0), torch.stack(ss).mean(0)
    det = boxes[:nd].contiguous()
    drois = K.tta_view_rois(det, table, V, H, W)
    logits = torch.randn(V, nd, S, S, device='cuda') * 3
    pred = torch.randn(4 * V * nd, 2, device='cuda')

    def base_masks():
        aug = []
        for v, d in enumerate(dirs):
            p = logits[v].sigmoid().cpu().numpy()
            aug.append(p if d is None else (p[:, :, ::-1] if d == 'horizontal' else p[:, ::-1, :]))
        merged = torch.from_numpy(np.mean(aug, axis=0)).cuda()
        return K.mask_paste(torch.logit(merged), det, H, W, 0.5)           # (paste of the merged probabilities)

    def base_offsets():
        p4 = pred.view(4, V, nd, 2)
        outs = []
        for v, d in enumerate(dirs):
            o = K.foa_fuse_decode(p4[:, v].reshape(-1, 2).contiguous(), drois[v * nd:(v + 1) * nd, 1:])
            outs.append(o if d is None else o * o.new_tensor([-1., 1.] if d == 'horizontal' else [1., -1.]))
        return torch.stack(outs).mean(0)
    stages = [('view_rois      n=1000', lambda: K.tta_view_rois(boxes, table, V, H, W), base_rois),
              ('merge_bboxes   n=1000', lambda: K.tta_merge_bboxes(rois, bp, cs, V, table, H, W, means, stds), base_bboxes),
              ('paste_views    n=100 ', lambda: K.mask_paste_views(logits, det, table, H, W), base_masks),
              ('merge_offsets  n=100 ', lambda: K.tta_merge_offsets(pred, drois, V, table), base_offsets)]
    lines.append('# merge stages at V = 3: fused kernel | torch-op per-view loop (baseline) | ratio')
    slower = []
    for name, fused, base in stages:
        tf, tb = timed(fused), timed(base)
        lines.append(f'{name}  {tf:8.3f} ms | {tb:8.3f} ms | x{tb / tf:.1f}')
        if tf > tb:
            slower.append(name)
    lines.append('expectation (no fused merge slower than its baseline): ' + ('holds' if not slower else f'FAILS for {slower}'))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
