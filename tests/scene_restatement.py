"""The merge rule of bonai_amd/scene.py restated in plain numpy, sharing no code with it: boxes translated to the scene frame, one
bitmap per detection, pair counts by ``&`` and sum, the greedy loop in priority order.

bitmaps_np    the paste rule transcribed to numpy (mask_rle_restatement.paste_np on sigmoid taps).  numpy's exp is not the device's
              expf, so the GPU tests hand the device's own ``kernels.mask_paste`` bitmaps to ``pair_counts`` instead.
windows       the integer paste windows (the bounds paste_outside leaves in)
pair_counts   (area [N], {(i, j): inter}) over the pairs i < j of different tiles whose windows intersect
truncated     a box side within ``border`` pixels of a tile edge that is not a scene edge
greedy        keep [N]: walk by priority (untruncated, then higher score, then lower index); a detection is suppressed iff a KEPT
              detection of higher priority shares an edge with it; edge iff inter > merge_thr * min(area_i, area_j), strictly
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_rle_restatement as M  # noqa: E402

f32 = np.float32


def translate(boxes, tiles, origins):
    """tile-frame boxes [N,4] + the origin (x0, y0) of each one's tile, in float32."""
    o = np.asarray(origins, f32)[np.asarray(tiles, np.int64)]
    return (np.asarray(boxes, f32) + np.concatenate([o, o], 1)).astype(f32)


def bitmaps_np(logits, boxes, H, W, thr=0.5):
    return np.stack([M.paste_np(M.sigmoid_np(l), b, H, W, thr) for l, b in zip(logits, boxes)]) if len(boxes) else \
        np.zeros((0, H, W), bool)


def windows(boxes, H, W):
    """int [N,4] = (x0, x1, y0, y1), half-open; empty when x0 >= x1 or y0 >= y1."""
    b = np.asarray(boxes, f32).reshape(-1, 4)
    with np.errstate(all='ignore'):
        x0 = np.minimum(np.maximum(np.floor(b[:, 0]) - 1, 0), W)
        x1 = np.maximum(np.minimum(np.ceil(b[:, 2]) + 1, W), 0)
        y0 = np.minimum(np.maximum(np.floor(b[:, 1]) - 1, 0), H)
        y1 = np.maximum(np.minimum(np.ceil(b[:, 3]) + 1, H), 0)
    return np.stack([x0, x1, y0, y1], 1).astype(np.int64)


def windows_meet(wa, wb):
    return max(wa[0], wb[0]) < min(wa[1], wb[1]) and max(wa[2], wb[2]) < min(wa[3], wb[3])


def pair_counts(bitmaps, boxes, tiles):
    bm = np.asarray(bitmaps).astype(bool)
    N, H, W = bm.shape
    win = windows(boxes, H, W)
    area = bm.reshape(N, -1).sum(1).astype(np.int64)
    recs = {}
    for i in range(N):
        for j in range(i + 1, N):
            if tiles[i] != tiles[j] and windows_meet(win[i], win[j]):
                recs[(i, j)] = int((bm[i] & bm[j]).sum())
    return area, recs


def truncated(boxes, tiles, origins, tile, H, W, border=2):
    th, tw = tile
    out = np.zeros(len(boxes), bool)
    for n, (b, t) in enumerate(zip(np.asarray(boxes, f32), tiles)):
        ox, oy = (int(v) for v in origins[int(t)])
        w, h = min(tw, W - ox), min(th, H - oy)
        out[n] = ((b[0] <= border and ox > 0) or (b[1] <= border and oy > 0) or
                  (b[2] >= w - border and ox + tw < W) or (b[3] >= h - border and oy + th < H))
    return out


def greedy(records, area, scores, trunc, merge_thr=0.5):
    """records: {(i, j): inter} or rows (i, j, inter) -> keep bool [N]."""
    rows = [(i, j, c) for (i, j), c in records.items()] if isinstance(records, dict) else [tuple(int(v) for v in r) for r in records]
    N = len(area)
    scores = np.asarray(scores, f32)
    nbr = [[] for _ in range(N)]
    for i, j, c in rows:
        m = min(int(area[i]), int(area[j]))
        if m > 0 and float(c) > float(merge_thr) * float(m):
            nbr[i].append(j)
            nbr[j].append(i)
    order = sorted(range(N), key=lambda n: (bool(trunc[n]), -float(scores[n]), n))
    keep = np.zeros(N, bool)
    seen = np.zeros(N, bool)
    for n in order:
        keep[n] = not any(seen[m] and keep[m] for m in nbr[n])
        seen[n] = True
    return keep


def merge(bitmaps, boxes_scene, boxes_tile, tiles, scores, origins, tile, H, W, merge_thr=0.5, border=2):
    area, recs = pair_counts(bitmaps, boxes_scene, tiles)
    return greedy(recs, area, scores, truncated(boxes_tile, tiles, origins, tile, H, W, border), merge_thr)
