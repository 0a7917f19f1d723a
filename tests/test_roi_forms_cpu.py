"""CPU: the RoIAlign forms (csrc/roi_align.hip) without a GPU -- the FORMS table tests/test_roi_forms_gpu.py runs, the built RoI lists with
their census, the float64 reference against the C oracle, what the entry points refuse, and a pin of what ROI_AUTO gives a bench
step's three lists.

The reference (reference_fwd / reference_bwd) is the defining sums of mmcv-1.0.5 RoIAlign (aligned=True, avg, adaptive grid) regrouped
per axis: a sample is valid iff its row AND its column are, and its bilinear weight is hat(y) hat(x), so
    out[py, px, c] = 1 / count  sum_y sum_x WY[py][y] WX[px][x] f[y, x, c],      WY[py][y] = sum over the bin row's valid sample rows
of the clamped hat weight of map row y.  Sample positions are formed in fp32 exactly as roi_geom and the kernels form them
(start + p * bin + (i + .5f) * bin / grid, every operation rounded, no contraction) so that the strict predicates, the clamps and
the truncation agree on both sides; everything after the position is float64.

Lists are built, not drawn: make_list(name) -> rois [K, 5] fp32; census(name, ...) counts the classes from the finished list through
K.roi_fwd_form (the launch path's own per-RoI decision, host only) and the reference's own axis tables.  Lattice lists ('L7', 'L14',
'crowd', 'one16'): map-space starts are multiples of 1/4 and bins are in {1/4, 1/2, 1, 2, 4, 8}; 'R7', 'R14' are the same RoIs moved off
the lattice plus a RoI over the whole map.  'fine' is a lattice list on a 1/64-pixel lattice (bins of a quarter pixel): its weights need
up to 12 significant bits, more than one 16-bit piece of the MFMA backward's two-piece weight holds, and stay exact in fp32; its 12
RoIs at two workgroups per RoI make an unordered grid that is a multiple of 8.  'tall' and 'wide' are one-level 66 x 3 and 3 x 66 maps
(fewer pixels than 19 x 17) whose RoIs reach footprints of 64 (tables fit) and 65 (> RF_MAX: sample loop) rows / columns.
Level boundaries: sqrt(w h) / 56 stays 1e-3 (relative) away from 2, 4 and 8 -- where floor(log2) changes the level (below 2 every value
is level 0) -- since log2f may differ by an ulp between host and device.  The sample loop is also reached through sub-pixel bins where no
LDS block exists (C = 72 / 192 / 320, and staging switched off)."""
import functools
import os

import numpy as np
import pytest
import torch

from bonai_amd import kernels as K
from bonai_amd import lib as L

F = np.float32
B = 2
STRIDES = [4, 8, 16, 32]
HW = [(19, 17), (10, 9), (5, 5), (3, 3)]          # tiles of 8: 3x3 + 2x2 + 1 + 1 = 15 per image, 30 in all: no multiple of 8
HW16, STRIDES16 = [(16, 16)], [4]                  # one level, 2 x 2 tiles x 2 images = 8: the XCD remap of the backward is on
FS = 56
assert (B * sum(-(-h // 8) * -(-w // 8) for h, w in HW)) % 8 != 0 and (B * 4) % 8 == 0


ONE_LEVEL = {'one16': (16, 16), 'tall': (66, 3), 'wide': (3, 66)}


def maps_of(name):
    return ([ONE_LEVEL[name]], STRIDES16) if name in ONE_LEVEL else (HW, STRIDES)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def roi_level(roi, num_levels):
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = np.sqrt(F(F(roi[3] - roi[1]) * F(roi[4] - roi[2])))
        lv = np.floor(np.log2(F(F(scale / F(FS)) + F(1e-6))))
    if np.isnan(lv):
        return 0                                   # fmaxf(NaN, 0) = 0
    return int(min(max(lv, 0), num_levels - 1))


def geom(roi, P, strides):
    """roi_geom in fp32 -> dict(batch, level, start_h, start_w, bin_h, bin_w, grid_h, grid_w, count)."""
    roi = np.asarray(roi, dtype=F)
    lv = roi_level(roi, len(strides)) if len(strides) > 1 else 0
    s = F(1.0 / strides[lv])
    sw, sh = F(F(roi[1] * s) - F(.5)), F(F(roi[2] * s) - F(.5))
    ew, eh = F(F(roi[3] * s) - F(.5)), F(F(roi[4] * s) - F(.5))
    rw, rh = F(ew - sw), F(eh - sh)
    bh, bw = F(rh / F(P)), F(rw / F(P))
    gh, gw = int(np.ceil(bh)), int(np.ceil(bw))
    return dict(batch=int(roi[0]), level=lv, start_h=sh, start_w=sw, bin_h=bh, bin_w=bw, grid_h=gh, grid_w=gw, count=max(gh * gw, 1))


def positions(start, bin_, grid, P):
    """fp32 sample positions [P, grid] of one axis, as the kernels round them."""
    p = np.arange(P, dtype=F)[:, None]
    i = np.arange(max(grid, 0), dtype=F)[None, :]
    return (F(start) + p * F(bin_)).astype(F) + ((i + F(.5)) * F(bin_)).astype(F) / F(max(grid, 1))


def axis_table(start, bin_, grid, P, size):
    """-> (W float64 [P, size]: summed hat weights, nvalid [P], pos fp32 [P, grid])."""
    pos = positions(start, bin_, grid, P)
    assert pos.dtype == F
    Wt, nv = np.zeros((P, size)), np.zeros(P, dtype=np.int64)
    for p in range(P):
        for v in pos[p]:
            if v < F(-1.0) or v > F(size):
                continue
            v = max(v, F(0))
            lo = int(v)
            if lo >= size - 1:
                lo = hi = size - 1
                v = F(lo)
            else:
                hi = lo + 1
            frac = float(v) - lo                   # exact: the fp32 difference is
            Wt[p, lo] += 1.0 - frac
            Wt[p, hi] += frac
            nv[p] += 1
    return Wt, nv, pos


def tables(roi, P, hw, strides):
    g = geom(roi, P, strides)
    H, W = hw[g['level']]
    g['WY'], g['nvy'], g['ys'] = axis_table(g['start_h'], g['bin_h'], g['grid_h'], P, H)
    g['WX'], g['nvx'], g['xs'] = axis_table(g['start_w'], g['bin_w'], g['grid_w'], P, W)
    return g


def reference_fwd(feats, rois, P, hw, strides, n_rot=1):
    """feats: float64 [B, H, W, C] per level.  -> dict(out, mag, n) each [n_rot K, P, P, C] (n: [.., 1]): the defining sums, the same
    sums over absolute values, the number of (sample, corner) terms."""
    Kn, C = len(rois), feats[0].shape[-1]
    out, mag, n = np.zeros((Kn, P, P, C)), np.zeros((Kn, P, P, C)), np.zeros((Kn, P, P, 1))
    for k, roi in enumerate(rois):
        g = tables(roi, P, hw, strides)
        f = feats[g['level']][g['batch']]
        out[k] = np.einsum('py,yxc,qx->pqc', g['WY'], f, g['WX']) / g['count']
        mag[k] = np.einsum('py,yxc,qx->pqc', g['WY'], np.abs(f), g['WX']) / g['count']
        n[k, :, :, 0] = 4 * np.outer(g['nvy'], g['nvx'])
    rot = lambda a: np.concatenate([np.rot90(a, r, axes=(1, 2)) for r in range(n_rot)])       # noqa: E731
    return dict(out=rot(out), mag=rot(mag), n=rot(n))


def unrotated_sum(g, n_rot):
    """g [n_rot K, P, P, C] -> [K, P, P, C]: the sum of the un-rotated gradients."""
    Kn = g.shape[0] // n_rot
    return sum(np.rot90(g[r * Kn:(r + 1) * Kn], -r, axes=(1, 2)) for r in range(n_rot))


def reference_bwd(gout, rois, P, hw, strides, C, n_rot=1, nb=B):
    """gout float64 [n_rot K, P, P, C] -> dict(grad, mag, n): per level [B, H, W, C] ([.., 1] for n = terms landing on the pixel)."""
    grad = [np.zeros((nb, h, w, C)) for h, w in hw]
    mag = [np.zeros((nb, h, w, C)) for h, w in hw]
    n = [np.zeros((nb, h, w, 1)) for h, w in hw]
    gs, ga = unrotated_sum(gout, n_rot), unrotated_sum(np.abs(gout), n_rot)
    for k, roi in enumerate(rois):
        g = tables(roi, P, hw, strides)
        lv, b = g['level'], g['batch']
        grad[lv][b] += np.einsum('py,pqc,qx->yxc', g['WY'], gs[k], g['WX']) / g['count']
        mag[lv][b] += np.einsum('py,pqc,qx->yxc', g['WY'], ga[k], g['WX']) / g['count']
        n[lv][b, :, :, 0] += n_rot * np.outer((g['WY'] != 0).sum(0), (g['WX'] != 0).sum(0))
    return dict(grad=grad, mag=mag, n=n)


# ---- the lists ---------------------------------------------------------------------------------------------------------------------
def _roi(b, lv, sx, sy, bw, bh, P, strides, hw):
    """A RoI of image b whose map-space start is (sx, sy) and whose bins are bw x bh pixels of level lv's map."""
    s = strides[lv]
    r = [b, (sx + .5) * s, (sy + .5) * s, (sx + .5 + P * bw) * s, (sy + .5 + P * bh) * s]
    g = geom(r, P, strides)
    assert g['level'] == lv and g['start_w'] == F(sx) and g['start_h'] == F(sy) and g['bin_w'] == F(bw) and g['bin_h'] == F(bh), (r, g)
    return r


# (image, level, sx, sy, bin_w, bin_h) in map pixels; comments: what the row is there for (at C = 256, shipped tuning)
L7 = [
    (1, 0, 2.75, 0, .5, .5),        # LDS: footprint 6 x 8 = 48 -> channel block 256
    (1, 0, 2, 2, .5, .5),           # LDS: 7 x 7 = 49 -> 128
    (1, 0, 2, 0, 2, .5),            # LDS: 6 x 16 = 96 -> 128; grid 1 x 2
    (1, 0, 2, 2, 2, .5),            # LDS: 7 x 16 = 112 -> 64
    (1, 0, 9, 11, .25, .25),        # LDS: 5 x 5, bins of a quarter pixel
    (1, 0, 3, -1.25, .5, .5),       # a sample row at exactly -1.0 (valid, row 0 at weight 1), then (-1, 0)
    (1, 0, 13.75, 3, .5, .5),       # a sample column at exactly W = 17.0 (valid, column 16 at weight 1)
    (1, 0, -1.5, 15.5, .5, .5),     # columns at -1.25 (invalid); rows in (H - 1, H)
    (1, 0, 5, 16, .5, .5),          # rows ... 19.25 = H + .25 (invalid): the last bin row has no valid sample
    (1, 0, 2, -3, 1, 8),            # walk (grid 8 x 1 > 4): rows of 6, 9, 6 and 0 contributing rows; bin_w exactly 1; Fw = 10
    (1, 0, 2.25, -4, 1, 8),         # walk: 5, 9 (10 with the fractional start), 7, 0 rows; Fw = 11 (odd)
    (1, 0, 3, .5, 1, 8),            # walk: 8 rows (samples on the rows themselves)
    (1, 0, 1, .5, 2, 4),            # walk: 4 rows; a sample at exactly H = 19.0 in bin row 4; bin rows 5, 6 off the map
    (1, 0, 1, 1, 2, 4),             # walk: 5 rows
    (1, 0, -2, 1, 4, 2),            # walk: 3 rows; grid 2 x 4; bin columns off the map on the right: xhi = -1
    (1, 0, -3, .5, 8, 1),           # walk: 1 row; bin columns 3 .. 6 have no valid sample
    (1, 0, -3, 1, 8, 1),            # walk: 2 rows
    (1, 0, 4, 4, 1, 1),             # bins of exactly one pixel: LDS at the shipped tuning, the walk with staging off
    (1, 0, 40, 40, 1, 1),           # wholly off the map
    (1, 0, 5, 5, 0, 0),             # zero size
    (1, 0, 9, 3, -.5, .5),          # reversed: x2 < x1
    (1, 1, -2, -4, 2, 4),           # level 1 (10 x 9), the whole map of that level inside the RoI
    (1, 2, -4, -2, 4, 2),           # level 2 (5 x 5); level 3 stays empty, and so does image 0
]
L14 = [
    (0, 0, 2, 8, 2, 1),             # LDS: footprint 12 x 16 = 192 -> 64 (grid 1 x 2 <= 4)
    (0, 0, 2, 7, 2, 1),             # 13 x 16 = 208 > 192: the walk
    (1, 0, 9, 9, .25, .25),         # 196 bins in one tile: seven operand chunks of the MFMA backward
    (1, 0, 4.25, 1.75, .25, .25),
    (0, 0, 8.75, 2, .5, .5),        # footprint reaches into tile column 0 (x0 = 7) without any weight there
    (0, 0, 1, -1.25, .5, .5),       # exactly -1.0
    (1, 0, 10.25, 12.25, .5, .5),   # exactly W and exactly H
    (0, 0, -3, 2, 2, .25),          # grid 1 x 2, columns off the map on the left
    (1, 0, 1, 1, 1, .5),            # bin_w exactly 1, sub-pixel rows
    (0, 0, 30, 30, .5, .5),         # off the map
    (0, 0, 3, 3, 0, 0),             # zero size
    (1, 0, 6, 2, -.25, .5),         # reversed
    (0, 1, -2, 1, 1, 2),            # level 1
    (1, 2, -5, -3, 2, 1),           # level 2
]


def _crowd(n):
    """n RoIs of image 1 on tile (1, 1) of the stride-4 map, bins of half a pixel, starts stepping through the quarter lattice."""
    return [(1, 0, 8 + (i % 13) * .25, 8 + (i // 13 % 11) * .25, .5, .5) for i in range(n)] + [(0, 0, 1, 1, .5, .5)]


def _one16():
    rows = [(b, 0, sx, sy, bw, bh) for b in (0, 1) for sx, sy, bw, bh in
            ((1, 1, .5, .5), (6.25, 5.5, .5, 1), (-1.25, 9, .5, .5), (3, 2, 1, 2), (9.75, 10.75, .5, .5))]
    return rows + [(1, 0, 2, 3, .25, .25)]          # K = 11: K, 2 K and 3 K are no multiples of 8


def _fine():
    """12 RoIs on the 1 / 64 lattice, bins of a quarter pixel, both images, sorted by image; tiles (0, 0), (1, 1) and the partial ones."""
    return [(i // 6, 0, 1 + 2.5 * (i % 6) + (2 * i + 1) / 64, 2 + 3 * (i % 5) + (62 - 5 * i) / 64, .25, .25) for i in range(12)]


def _narrow(tall):
    """(start along the long axis, bin along the short axis): the RoI runs off the far end of the 66-pixel axis (bins of 8 at P = 14), so
    its footprint is 65 - floor(start - 1) + 1: start 3 -> 64, start 2 -> 65."""
    rows = []
    for b, start, short in ((0, 3, .25), (1, 2, .25), (0, 3, 1), (1, 2, 1), (1, 3.25, .5), (0, 2.25, .5), (0, 30, .25)):
        rows.append((b, 0, -.25, start, short, 8) if tall else (b, 0, start, -.25, 8, short))
    return rows


LISTS = {'fine': (_fine(), 7), 'tall': (_narrow(True), 14), 'wide': (_narrow(False), 14), 'L7': (L7, 7), 'L14': (L14, 14), 'crowd257': (_crowd(257), 7), 'crowd513': (_crowd(513), 7), 'one16': (_one16(), 7)}
LATTICE = tuple(LISTS)
RANDOM = ('R7', 'R14')


@functools.lru_cache(maxsize=None)
def make_list(name):
    """-> (rois fp32 [K, 5], P)."""
    hw, strides = maps_of(name)
    if name in LISTS:
        rows, P = LISTS[name]
        return np.array([_roi(b, lv, sx, sy, bw, bh, P, strides, hw) for b, lv, sx, sy, bw, bh in rows], dtype=F), P
    base, P = make_list('L' + name[1:])
    gen = np.random.RandomState(70 + P)
    rois = base.copy()
    live = (rois[:, 3] != rois[:, 1])
    rois[live, 1:] += gen.uniform(-1.5, 1.5, (int(live.sum()), 4)).astype(F)          # off the lattice; sizes change by < 3 pixels of the image
    rois[:, 0] = np.arange(len(rois)) % B                                              # both images
    whole = np.array([[0, 0, 0, 4 * 17, 4 * 19], [1, 0, 0, 4 * 17, 4 * 19]], dtype=F)  # a RoI over the whole (stride-4) map
    return np.concatenate([rois, whole[:1 if (len(rois) + 1) % 8 else 2]]).astype(F), P       # K stays off the multiples of 8


def level_margin(rois):
    """Smallest relative distance of sqrt(w h) / 56 from a level boundary (2, 4, 8) over the RoIs of positive area."""
    w, h = rois[:, 3] - rois[:, 1], rois[:, 4] - rois[:, 2]
    ok = (w > 0) & (h > 0)
    r = np.sqrt(w[ok].astype(np.float64) * h[ok]) / FS
    return min(np.abs(r / t - 1).min() for t in (2, 4, 8))


def forms_of(name, C, dtype, variant=K.ROI_AUTO):
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    return [K.roi_fwd_form(hw, strides, C, dtype, r, len(rois), P, FS, variant) for r in rois]


def census(name, C=256, variant=K.ROI_AUTO):
    """Counts of the classes, from the finished list (forms: the host query at C channels of the 16-bit type)."""
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    c = dict.fromkeys(('at_minus_1', 'at_size', 'beyond_low', 'beyond_high', 'strip_low', 'strip_high', 'bin_without_sample',
                       'bin_row_without_sample', 'off_map', 'zero_size', 'reversed', 'grid_h_ne_grid_w', 'bin_w_1', 'odd_Fw_walk',
                       'even_Fw_walk', 'touch_without_weight', 'chunks_gt_1', 'whole_map'), 0)
    c.update(images=set(), levels=set(), lds=set(), walk_nrow=set(), loop=0, walk=0)
    for roi, form in zip(rois, forms_of(name, C, L.act16(), variant)):
        g = tables(roi, P, hw, strides)
        H, W = hw[g['level']]
        kern, fm, cbch, Fh, Fw, _ = form
        allv = np.concatenate([g['ys'].ravel(), g['xs'].ravel()])
        sizes = np.concatenate([np.full(g['ys'].size, H), np.full(g['xs'].size, W)])
        live = g['nvy'].sum() > 0 and g['nvx'].sum() > 0
        c['at_minus_1'] += int((allv == -1).any())
        c['at_size'] += int((allv == sizes).any())
        c['beyond_low'] += int(live and ((allv < -1) & (allv >= -1.5)).any())
        c['beyond_high'] += int(live and ((allv > sizes) & (allv <= sizes + .5)).any())
        c['strip_low'] += int(((allv > -1) & (allv < 0)).any())
        c['strip_high'] += int(((allv > sizes - 1) & (allv < sizes)).any())
        c['bin_without_sample'] += int(live and ((g['nvy'] == 0).any() or (g['nvx'] == 0).any()))
        c['bin_row_without_sample'] += int(live and (g['nvy'] == 0).any())
        c['off_map'] += int(g['grid_h'] > 0 and g['grid_w'] > 0 and not live)
        c['zero_size'] += int(roi[3] == roi[1] and roi[4] == roi[2])
        c['reversed'] += int(roi[3] < roi[1])
        c['whole_map'] += int(g['start_w'] <= 0 and g['start_h'] <= 0 and g['start_w'] + g['bin_w'] * P >= W - 1
                              and g['start_h'] + g['bin_h'] * P >= H - 1)
        c['grid_h_ne_grid_w'] += int(live and g['grid_h'] != g['grid_w'])
        c['bin_w_1'] += int(live and g['bin_w'] == 1 and fm == K.ROI_FORM_WALK)
        c['images'].add(g['batch'])
        c['levels'].add(g['level'])
        if fm == K.ROI_FORM_LDS:
            c['lds'].add((cbch, Fh * Fw))
        elif fm == K.ROI_FORM_LOOP:
            c['loop'] += 1
        else:
            c['walk'] += 1
            c['odd_Fw_walk' if Fw % 2 else 'even_Fw_walk'] += 1
            for p in range(P):                     # contributing rows of bin row p: first to last, as the kernel's ballots find them
                nz = np.flatnonzero(g['WY'][p])
                c['walk_nrow'].add(int(nz[-1] - nz[0] + 1) if len(nz) else 0)
        # backward: (RoI, 8 x 8 tile) pairs
        if g['grid_h'] > 0 and g['grid_w'] > 0:
            x0, x1 = int(np.floor(np.clip(min(g['start_w'], g['start_w'] + g['bin_w'] * P) - 1, 0, W - 1))), \
                int(np.ceil(np.clip(max(g['start_w'], g['start_w'] + g['bin_w'] * P) + 1, 0, W - 1)))
            y0, y1 = int(np.floor(np.clip(min(g['start_h'], g['start_h'] + g['bin_h'] * P) - 1, 0, H - 1))), \
                int(np.ceil(np.clip(max(g['start_h'], g['start_h'] + g['bin_h'] * P) + 1, 0, H - 1)))
            assert (Fh, Fw) == (y1 - y0 + 1, x1 - x0 + 1), (roi, form)
            for ty in range(y0 // 8, y1 // 8 + 1):
                for tx in range(x0 // 8, x1 // 8 + 1):
                    rows = (g['WY'][:, ty * 8:ty * 8 + 8] != 0).any(1).sum()
                    cols = (g['WX'][:, tx * 8:tx * 8 + 8] != 0).any(1).sum()
                    c['touch_without_weight'] += int(rows * cols == 0)
                    c['chunks_gt_1'] += int(rows * cols > 32)
    return c


# ---- the table the GPU file runs -----------------------------------------------------------------------------------------------
# (id, forced kernel, C, type '16' | '32', P, n_rot, tuning of the 16-byte kernel, ordered launch, kernel the row reaches)
_T = K.roi_fwd_variant
FORMS = [
    ('sample_f32_c64', K.ROI_AUTO, 64, '32', 7, 1, {}, False, K.ROI_KERNEL_SAMPLE_F32),
    ('sample_f32_c72_p14_rot4', K.ROI_AUTO, 72, '32', 14, 4, {}, True, K.ROI_KERNEL_SAMPLE_F32),
    ('sample16_c64', K.ROI_FWD_SAMPLE, 64, '16', 7, 1, {}, False, K.ROI_KERNEL_SAMPLE_16),
    ('sep4_c64', K.ROI_FWD_SEP4, 64, '16', 7, 1, {}, False, K.ROI_KERNEL_SEP4),
    ('sep4_c68_partial_lanes', K.ROI_AUTO, 68, '16', 7, 4, {}, True, K.ROI_KERNEL_SEP4),
    ('sep4_c256_p14', K.ROI_FWD_SEP4, 256, '16', 14, 1, {}, False, K.ROI_KERNEL_SEP4),
    ('sep8_c256', K.ROI_AUTO, 256, '16', 7, 1, {}, False, K.ROI_KERNEL_SEP8),
    ('sep8_c256_rot4_ordered', K.ROI_AUTO, 256, '16', 7, 4, {}, True, K.ROI_KERNEL_SEP8),
    ('sep8_c256_p14', K.ROI_AUTO, 256, '16', 14, 1, {}, False, K.ROI_KERNEL_SEP8),
    ('sep8_c256_p14_rot4', K.ROI_AUTO, 256, '16', 14, 4, {}, False, K.ROI_KERNEL_SEP8),
    ('sep8_c256_no_stage', K.ROI_AUTO, 256, '16', 7, 1, dict(stage_kib=255), False, K.ROI_KERNEL_SEP8),
    ('sep8_c256_p14_no_stage', K.ROI_AUTO, 256, '16', 14, 1, dict(stage_kib=255), False, K.ROI_KERNEL_SEP8),
    ('sep8_c256_nsplit1', K.ROI_AUTO, 256, '16', 7, 1, dict(nsplit=1), False, K.ROI_KERNEL_SEP8),
    ('sep8_c256_nsplit3_rot4', K.ROI_AUTO, 256, '16', 7, 4, dict(nsplit=3), False, K.ROI_KERNEL_SEP8),
    ('sep8_c256_gmax15_stage64', K.ROI_AUTO, 256, '16', 7, 1, dict(stage_kib=64, gmax=15), False, K.ROI_KERNEL_SEP8),
    ('sep8_c64', K.ROI_AUTO, 64, '16', 7, 1, {}, False, K.ROI_KERNEL_SEP8),
    ('sep8_c512', K.ROI_AUTO, 512, '16', 7, 1, {}, False, K.ROI_KERNEL_SEP8),
    ('sep8_c72_partial_lanes', K.ROI_AUTO, 72, '16', 7, 1, {}, False, K.ROI_KERNEL_SEP8),
    ('sep8_c320_two_passes', K.ROI_AUTO, 320, '16', 7, 1, {}, False, K.ROI_KERNEL_SEP8),
    ('sep8_c192_p14', K.ROI_AUTO, 192, '16', 14, 1, {}, False, K.ROI_KERNEL_SEP8),
]
FORM_IDS = [r[0] for r in FORMS]
# backward: (id, variant, C, operand type, gradient-map type, P, n_rot, kernel the row reaches)
BWD_FORMS = [
    ('valu_f32_c64', K.ROI_AUTO, 64, '32', '32', 7, 1, 'tile<f32,f32>'),
    ('valu_f32_c72_p14_rot4', K.ROI_AUTO, 72, '32', '32', 14, 4, 'tile<f32,f32>'),
    ('valu_16_f32_c256', K.ROI_AUTO, 256, '16', '32', 7, 1, 'tile<16,f32>'),
    ('valu_16_16_c64', K.ROI_AUTO, 64, '16', '16', 7, 4, 'tile<16,16>'),
    ('valu_16_16_c256_forced_p14', K.ROI_BWD_VALU, 256, '16', '16', 14, 1, 'tile<16,16>'),
    ('valu_16_16_c320', K.ROI_AUTO, 320, '16', '16', 7, 1, 'tile<16,16>'),
    ('mfma_p7', K.ROI_AUTO, 256, '16', '16', 7, 1, 'mfma'),
    ('mfma_p7_rot4', K.ROI_AUTO, 256, '16', '16', 7, 4, 'mfma'),
    ('mfma_p14', K.ROI_AUTO, 256, '16', '16', 14, 1, 'mfma'),
    ('mfma_p14_rot4', K.ROI_AUTO, 256, '16', '16', 14, 4, 'mfma'),
    ('pipe_p7', K.ROI_BWD_PIPE, 256, '16', '16', 7, 1, 'pipe'),
    ('pipe_p14', K.ROI_BWD_PIPE, 256, '16', '16', 14, 1, 'pipe'),
    ('pipe_p14_rot4', K.ROI_BWD_PIPE, 256, '16', '16', 14, 4, 'pipe'),
]
BWD_IDS = [r[0] for r in BWD_FORMS]


def dtype_of(kind):
    return torch.float32 if kind == '32' else L.act16()


def variant_of(row):
    return _T(row[1], **row[6])


def list_of(row, lattice=True):
    return ('L' if lattice else 'R') + str(row[4])


@pytest.fixture(scope='module', autouse=True)
def _library():
    if not (os.path.exists(L._LIB_PATH) and os.path.exists(L._LIB_PATH_F16)):
        from bonai_amd import build
        build.build()


# ---- tests -------------------------------------------------------------------------------------------------------------------------
def test_codes():
    assert (K.ROI_KERNEL_SAMPLE_F32, K.ROI_KERNEL_SAMPLE_16, K.ROI_KERNEL_SEP4, K.ROI_KERNEL_SEP8) == (1, 2, 3, 4)
    assert (K.ROI_FORM_LDS, K.ROI_FORM_WALK, K.ROI_FORM_LOOP) == (1, 2, 3)
    assert _T(stage_kib=255, min_cb=1, gmax=5, nsplit=3) == 255 << 8 | 1 << 16 | 5 << 18 | 3 << 22


@pytest.mark.parametrize('name', LATTICE + RANDOM)
def test_levels_stay_clear_of_the_boundaries(name):
    rois, P = make_list(name)
    assert name in ONE_LEVEL or level_margin(rois) >= 1e-3          # (one level: no level rule)
    assert len(rois) % 8 != 0 or name.startswith('crowd')          # ordered launches pad the grid to a multiple of 8
    assert rois.dtype == F and rois.shape[1] == 5


@pytest.mark.parametrize('row', FORMS, ids=FORM_IDS)
def test_row_reaches_its_kernel(row):
    for lattice in (True, False):
        forms = forms_of(list_of(row, lattice), row[2], dtype_of(row[3]), variant_of(row))
        assert {f[0] for f in forms} == {row[8]}
        want_split = row[6].get('nsplit', 2) if row[8] == K.ROI_KERNEL_SEP8 else 1
        assert {f[5] for f in forms} == {want_split}
        if row[8] in (K.ROI_KERNEL_SAMPLE_F32, K.ROI_KERNEL_SAMPLE_16):
            assert {f[1:3] for f in forms} == {(K.ROI_FORM_LOOP, 0)}


def test_census_L7():
    c = census('L7')
    assert c['lds'] >= {(256, 48), (128, 49), (128, 96), (64, 112)}, c['lds']
    assert c['walk_nrow'] >= set(range(10)), c['walk_nrow']          # 0, 1 .. 8, and 9 = 8 + a second batch
    assert max(c['walk_nrow']) in (9, 10)
    for name in ('at_minus_1', 'at_size', 'beyond_low', 'beyond_high', 'strip_low', 'strip_high', 'bin_without_sample',
                 'bin_row_without_sample', 'off_map', 'zero_size', 'reversed', 'grid_h_ne_grid_w', 'bin_w_1', 'odd_Fw_walk',
                 'even_Fw_walk', 'walk', 'whole_map'):
        assert c[name] >= 1, (name, c)
    assert c['images'] == {1} and c['levels'] == {0, 1, 2}             # image 0 and level 3 get no RoI
    assert c['loop'] == 0
    rois, P = make_list('L7')
    assert P == 7 and len(rois) % 8 != 0 and (2 * len(rois)) % 8 != 0 and (3 * len(rois)) % 8 != 0
    # the walk at the shipped tuning comes from grid_h grid_w > 4 alone: the same RoIs, asked with gmax = 15 and room to stage, take LDS
    auto = forms_of('L7', 256, L.act16())
    roomy = forms_of('L7', 256, L.act16(), _T(stage_kib=64, gmax=15))
    assert any(a[1] == K.ROI_FORM_WALK and b[1] == K.ROI_FORM_LDS for a, b in zip(auto, roomy))
    # staging off: every RoI with bins of a pixel or more walks, the sub-pixel ones take the sample loop
    off = census('L7', variant=_T(stage_kib=255))
    assert not off['lds'] and off['loop'] >= 8 and off['walk'] > c['walk'] and off['bin_w_1'] > c['bin_w_1']
    # no LDS block exists for C = 72 / 320 (no power of two): walk | loop at the shipped tuning; C = 64 and 512 stage
    for C in (72, 320):
        cc = census('L7', C)
        assert not cc['lds'] and cc['loop'] >= 8 and cc['walk'] >= 8
    assert {b for b, _ in census('L7', 64)['lds']} == {64}
    assert {b for b, _ in census('L7', 512)['lds']} >= {512, 256, 128}
    # the 8-byte kernel: walk and sample loop
    s4 = {f[1] for f in forms_of('L7', 68, L.act16())}
    assert s4 == {K.ROI_FORM_WALK, K.ROI_FORM_LOOP}


def test_census_L14():
    c = census('L14')
    assert (64, 192) in c['lds'] and c['walk'] >= 1, c                 # 12 x 16 = 192 stages, 13 x 16 = 208 walks
    f14 = forms_of('L14', 256, L.act16())
    assert f14[0][1:5] == (K.ROI_FORM_LDS, 64, 12, 16) and f14[1][1:5] == (K.ROI_FORM_WALK, 0, 13, 16)
    for name in ('at_minus_1', 'at_size', 'strip_low', 'strip_high', 'off_map', 'zero_size', 'reversed', 'grid_h_ne_grid_w',
                 'touch_without_weight', 'chunks_gt_1'):
        assert c[name] >= 1, (name, c)
    assert c['images'] == {0, 1} and c['levels'] == {0, 1, 2}
    assert census('L14', 192)['loop'] >= 6                             # C = 192: no LDS block


@pytest.mark.parametrize('name,n', [('crowd257', 257), ('crowd513', 513)])
def test_census_crowd(name, n):
    """More than RB_LIST = 256 RoIs of one image on one tile: two and three batches of the tile owner's list."""
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    on_tile = 0
    for roi in rois:
        g = tables(roi, P, hw, strides)
        on_tile += int(g['batch'] == 1 and g['level'] == 0 and (g['WY'][:, 8:16] != 0).any() and (g['WX'][:, 8:16] != 0).any())
    assert on_tile == n and len(rois) == n + 1
    assert min(abs(float(r[3] - r[1])) for r in rois) / 4 / 7 >= .5    # bins of half a pixel or more


def significant_bits(x):
    """Bits from the leading to the trailing one of a dyadic number."""
    m, _ = np.frexp(abs(float(x)))
    n = 0
    while m != int(m):
        m *= 2
        n += 1
    return n


def test_census_fine():
    """Weights that one 16-bit piece cannot hold (bfloat16: 8 bits, binary16: 11), yet exact in fp32; an unordered grid of 8 n."""
    rois, P = make_list('fine')
    hw, strides = maps_of('fine')
    assert len(rois) % 8 != 0 and {f[5] for f in forms_of('fine', 256, L.act16())} == {2} and (2 * len(rois)) % 8 == 0
    assert (rois[1:, 0] >= rois[:-1, 0]).all() and set(rois[:, 0]) == {0, 1}
    most = 0
    for roi in rois:
        g = tables(roi, P, hw, strides)
        a = np.einsum('py,qx->pqyx', g['WY'], g['WX']) / g['count']
        most = max(most, max(significant_bits(v) for v in np.unique(a)))
    assert most > (8 if L.act16() == torch.bfloat16 else 11) and most == 12, most
    assert list_grain('fine') == 2.0 ** -12
    c = census('fine')
    assert c['chunks_gt_1'] >= 1 and c['images'] == {0, 1}


@pytest.mark.parametrize('name', ['tall', 'wide'])
def test_census_narrow(name):
    """Footprints of 64 rows / columns take the LDS form (sub-pixel bins across) or the walk; 65 take the sample loop, in both
    separable kernels."""
    ax = 3 if name == 'tall' else 4
    for C, variant, kern in ((256, K.ROI_AUTO, K.ROI_KERNEL_SEP8), (64, K.ROI_FWD_SEP4, K.ROI_KERNEL_SEP4)):
        got = {}
        for f in forms_of(name, C, L.act16(), variant):
            assert f[0] == kern
            got.setdefault(f[ax], set()).add(f[1])
        assert got[65] == {K.ROI_FORM_LOOP}, got
        assert got[64] == ({K.ROI_FORM_LDS, K.ROI_FORM_WALK} if kern == K.ROI_KERNEL_SEP8 else {K.ROI_FORM_WALK, K.ROI_FORM_LOOP}), got
        assert max(got) == 65


def test_census_one16():
    rois, P = make_list('one16')
    assert len(rois) == 11 and census('one16')['images'] == {0, 1}


def _oracle_fwd(feats, rois, P, hw, strides):
    from oracle import cops
    out = np.zeros((len(rois), P, P, feats[0].shape[-1]), dtype=F)
    lv = np.array([geom(r, P, strides)['level'] for r in rois])
    for i, s in enumerate(strides):
        if (lv == i).any():
            f = torch.from_numpy(feats[i]).permute(0, 3, 1, 2).float()
            out[lv == i] = cops.roi_align_fwd(f, torch.from_numpy(rois[lv == i]), P, 1.0 / s).permute(0, 2, 3, 1).numpy()
    return out


def _oracle_bwd(gout, rois, P, hw, strides, C):
    from oracle import cops
    lv = np.array([geom(r, P, strides)['level'] for r in rois])
    grads = []
    for i, s in enumerate(strides):
        g = torch.from_numpy(gout[lv == i]).permute(0, 3, 1, 2).float()
        grads.append(cops.roi_align_bwd(g, torch.from_numpy(rois[lv == i]), (B, C) + hw[i], 1.0 / s).permute(0, 2, 3, 1).numpy())
    return grads


def operands(name, C, lattice, kind='32', n_rot=1, unit=False):
    """-> (feats [B, H, W, C] per level, gout [n_rot K, P, P, C]) float64, already rounded to the operand type."""
    rois, P = make_list(name)
    hw, _ = maps_of(name)
    gen = torch.Generator().manual_seed(900 + C + 7 * P + n_rot + len(rois))
    dt = dtype_of(kind)
    if lattice:
        feats = [torch.randint(-4, 5, (B, h, w, C), generator=gen).double().numpy() for h, w in hw]
        lo, hi = (-1, 2) if unit else (-4, 5)
        gout = torch.randint(lo, hi, (n_rot * len(rois), P, P, C), generator=gen).double().numpy()
    else:
        feats = [torch.randn(B, h, w, C, generator=gen).to(dt).double().numpy() for h, w in hw]
        gout = torch.randn(n_rot * len(rois), P, P, C, generator=gen).to(dt).double().numpy()
    return feats, gout


def _pow2_grain(a):
    """The largest power of two (<= 1) of which every entry of `a` is an integer multiple."""
    g = 1.0
    while not np.array_equal(a / g, np.round(a / g)):
        g /= 2
        assert g >= 2.0 ** -8, 'not on the lattice'
    return g


@functools.lru_cache(maxsize=None)
def list_grain(name):
    """The power-of-two grain of every term a lattice list can produce from integer operands: per RoI the grain of its row table x the
    grain of its column table / count (a power of two), the smallest over the list.  The two 16-bit pieces of an MFMA weight are
    roundings of such a multiple to fewer bits, hence multiples of it too."""
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    g = 1.0
    for roi in rois:
        t = tables(roi, P, hw, strides)
        assert t['count'] in (1, 2, 4, 8, 16, 32, 64)
        g = min(g, _pow2_grain(t['WY']) * _pow2_grain(t['WX']) / t['count'])
    return g


def grain_ok(name, ref, mag):
    """Every term of every sum over list `name` is an integer multiple of g = list_grain(name); with sum|terms| / g < 2^24 every
    partial sum, in any order and grouping, is an integer multiple of g below 2^24 g: exact in fp32."""
    g = list_grain(name)
    return bool(np.all(ref / g == np.round(ref / g)) and mag.max() / g < 2 ** 24)


@pytest.mark.parametrize('name', ('L7', 'L14', 'one16', 'crowd257', 'fine', 'tall', 'wide'))
def test_reference_equals_the_oracle_on_the_lattice(name):
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    C = 8
    feats, gout = operands(name, C, True, unit=name.startswith('crowd'))
    R = reference_fwd(feats, rois, P, hw, strides)
    assert grain_ok(name, R['out'], R['mag'])
    assert np.array_equal(R['out'], _oracle_fwd(feats, rois, P, hw, strides).astype(np.float64))
    G = reference_bwd(gout, rois, P, hw, strides, C)
    for lv, (want, got) in enumerate(zip(G['grad'], _oracle_bwd(gout, rois, P, hw, strides, C))):
        assert grain_ok(name, want, G['mag'][lv])
        assert np.array_equal(want, got.astype(np.float64)), (name, lv)
    assert not G['grad'][3].any() if name in ('L7', 'L14') else True
    assert list_grain(name) >= 2.0 ** -12
    assert len(G['grad']) == len(hw)


@pytest.mark.parametrize('name', RANDOM)
def test_reference_within_fp32_rounding_of_the_oracle(name):
    """The oracle is the sample-order fp32 sum: hat weight 3 roundings (1 - l twice, their product), the product with the value 1,
    the division by count 1 -> c = 5, n = the (sample, corner) terms; backward: g / count 1, x weight 1, weight 3 -> c = 5."""
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    C, U = 8, 2.0 ** -24
    feats, gout = operands(name, C, False)
    R = reference_fwd(feats, rois, P, hw, strides)
    err = np.abs(_oracle_fwd(feats, rois, P, hw, strides) - R['out'])
    assert (err <= (R['n'] + 5) * U * R['mag']).all(), (err / ((R['n'] + 5) * U * R['mag'] + 1e-300)).max()
    G = reference_bwd(gout, rois, P, hw, strides, C)
    for lv, got in enumerate(_oracle_bwd(gout, rois, P, hw, strides, C)):
        assert (np.abs(got - G['grad'][lv]) <= _bwd_oracle_bound(G, lv, rois, P, strides)).all(), (name, lv)


def _bwd_oracle_bound(G, lv, rois, P, strides):
    """(n + 5) u mag with n = the oracle's own deposits on the pixel: per (RoI, bin) at most 4 corners x count samples."""
    gmax = max(max(geom(r, P, strides)['count'], 1) for r in rois)
    return (4 * gmax * G['n'][lv] + 5) * 2.0 ** -24 * G['mag'][lv]


# ---- refusals: hipErrorInvalidValue (1), nothing launched --------------------------------------------------------------------
def _fwd_code(C=64, dtype=None, P=7, n_rot=1, variant=0, Kn=4):
    """loft_roi_align_fwd_ord's return code.  A refusal returns before anything is launched or dereferenced: without a device the
    buffers are made-up addresses; with one they are real and large enough, so that a refusal that regressed fails the assert
    instead of running a kernel on wild pointers."""
    dtype = L.F32 if dtype is None else dtype
    from ctypes import c_float, c_int, c_void_p
    if torch.cuda.is_available():
        f = [torch.zeros(B * h * w * max(C, 8) * 2, device='cuda') for h, w in HW]
        rois, out = torch.zeros(Kn * 5, device='cuda'), torch.zeros(4 * Kn * 16 * 16 * max(C, 8), device='cuda')
        fp, rp, op = [t.data_ptr() for t in f], rois.data_ptr(), out.data_ptr()
    else:
        fp, rp, op = [1 << 20] * 4, 1 << 20, 1 << 20
    code = L.load().loft_roi_align_fwd_ord(L.arr(c_void_p, fp), L.arr(c_int, [h for h, _ in HW]), L.arr(c_int, [w for _, w in HW]),
                                           L.arr(c_float, [1.0 / s for s in STRIDES]), 4, FS, C, dtype, rp, Kn, P, n_rot, op, variant,
                                           None, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return code


def _bwd_code(C=64, dtype=None, grad_dtype=None, P=7, n_rot=1, variant=0, Kn=4):
    dtype = L.F32 if dtype is None else dtype
    grad_dtype = L.F32 if grad_dtype is None else grad_dtype
    from ctypes import c_float, c_int, c_void_p
    if torch.cuda.is_available():
        f = [torch.zeros(B * h * w * max(C, 8) * 2, device='cuda') for h, w in HW]
        rois, g = torch.zeros(Kn * 5, device='cuda'), torch.zeros(4 * Kn * 16 * 16 * max(C, 8), device='cuda')
        ws = torch.zeros(48 * Kn, device='cuda')
        fp, rp, gp, wp = [t.data_ptr() for t in f], rois.data_ptr(), g.data_ptr(), ws.data_ptr()
    else:
        fp, rp, gp, wp = [1 << 20] * 4, 1 << 20, 1 << 20, 1 << 20
    code = L.load().loft_roi_align_bwd_v(L.arr(c_void_p, fp), L.arr(c_int, [h for h, _ in HW]), L.arr(c_int, [w for _, w in HW]),
                                         L.arr(c_float, [1.0 / s for s in STRIDES]), 4, FS, C, dtype, rp, Kn, P, n_rot, gp, B, 0, 0, wp,
                                         grad_dtype, variant, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return code


FWD_REFUSALS = [
    ('kernel_code_3', dict(variant=3)), ('kernel_code_255', dict(variant=255)), ('stray_bit_25', dict(variant=1 << 25)),
    ('negative', dict(variant=-1)),
    ('tuning_with_sample', dict(variant=_T(K.ROI_FWD_SAMPLE, stage_kib=24))), ('nsplit_with_sep4', dict(variant=_T(K.ROI_FWD_SEP4, nsplit=2))),
    ('c_66', dict(C=66)), ('n_rot_2', dict(n_rot=2)), ('n_rot_0', dict(n_rot=0)),
]


@pytest.mark.parametrize('case', FWD_REFUSALS, ids=[c[0] for c in FWD_REFUSALS])
def test_forward_refusals(case):
    kw = dict(case[1])
    for dt in (L.F32, L._DT[L.act16()]):
        assert _fwd_code(dtype=dt, **kw) == 1
    if 'n_rot' not in kw:                          # the form query takes no rotation count; everything else it refuses alike
        with pytest.raises(L.LoftHipError):
            K.roi_fwd_form(HW, STRIDES, kw.get('C', 64), L.act16(), [0, 8, 8, 36, 36], 4, 7, FS, kw.get('variant', 0))


def test_form_query_refusals():
    other = torch.float16 if L.act16() == torch.bfloat16 else torch.bfloat16
    with pytest.raises(L.LoftHipError):
        K.roi_fwd_form(HW, STRIDES, 64, other, [0, 8, 8, 36, 36], 4, 7)
    with pytest.raises(L.LoftHipError):
        K.roi_fwd_form(HW, STRIDES, 64, L.act16(), [0, 8, 8, 36, 36], 0, 7)
    with pytest.raises(L.LoftHipError):
        K.roi_fwd_form(HW + [(2, 2)], STRIDES + [64], 64, L.act16(), [0, 8, 8, 36, 36], 4, 7)
    assert _fwd_code(dtype=L._DT[other]) == 1


BWD_REFUSALS = [
    ('kernel_code_3', dict(variant=3)), ('kernel_code_255', dict(variant=255)), ('c_66', dict(C=66)), ('n_rot_3', dict(n_rot=3)),
    ('p_15', dict(P=15)), ('16bit_map_fp32_operands', dict(grad_dtype='16')),
]


@pytest.mark.parametrize('case', BWD_REFUSALS, ids=[c[0] for c in BWD_REFUSALS])
def test_backward_refusals(case):
    kw = dict(case[1])
    if kw.get('grad_dtype') == '16':
        kw['grad_dtype'] = L._DT[L.act16()]
    assert _bwd_code(**kw) == 1
    if 'grad_dtype' not in kw:
        assert _bwd_code(dtype=L._DT[L.act16()], grad_dtype=L._DT[L.act16()], **kw) == 1


# ---- what ROI_AUTO resolves to for a bench step's three lists -------------------------------------------------------------------
def _bench_list(n, P):
    """A fixed list over the bench step's pyramid (8 x 1024^2: maps of 256, 128, 64, 32): RoI i is a square of side
    8 .. 153 image pixels (log-uniform in 64 steps), centred on a fixed stepping pattern."""
    i = np.arange(n)
    side = 8 * 20 ** ((i % 64) / 64)
    cx, cy = 40 + (i * 37 % 944), 40 + (i * 101 % 944)
    return np.stack([i % 8, cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2], 1).astype(F)


# (K, P, histogram {(form, cbch): RoIs}, nsplit).  Bins of a pixel or more start at side 28 (P = 7) and 56 (P = 14) image pixels;
# with the 24 KiB stage a footprint of <= 48 / 96 / 192 pixels takes channel block 256 / 128 / 64.  The numbers are the rule's, read off
# roi_sep8_form; moving the stage size, gmax = 4 or the K <= 4096 split rule changes them.
BENCH = [(8192, 7), (2048, 14), (2048, 7)]
_LDS, _WALK, _LOOP = K.ROI_FORM_LDS, K.ROI_FORM_WALK, K.ROI_FORM_LOOP
BENCH_HIST = {
    (8192, 7): {(_LDS, 256): 640, (_LDS, 128): 2176, (_LDS, 64): 1664, (_WALK, 0): 3712},
    (2048, 14): {(_LDS, 256): 160, (_LDS, 128): 544, (_LDS, 64): 416, (_LOOP, 0): 224, (_WALK, 0): 704},
    (2048, 7): {(_LDS, 256): 160, (_LDS, 128): 544, (_LDS, 64): 416, (_WALK, 0): 928},
}


def _bench_hist(Kn, P, variant=K.ROI_AUTO):
    hw = [(256, 256), (128, 128), (64, 64), (32, 32)]
    hist, splits = {}, set()
    for roi in _bench_list(Kn, P):
        kern, fm, cbch, Fh, Fw, ns = K.roi_fwd_form(hw, STRIDES, 256, L.act16(), roi, Kn, P, FS, variant)
        assert kern == K.ROI_KERNEL_SEP8
        hist[(fm, cbch)] = hist.get((fm, cbch), 0) + 1
        splits.add(ns)
    return hist, splits


def _expected_hist(Kn, P, stage=24 * 1024, gmax=4):
    """The dispatch rule written out a second time, from the reference's own geometry."""
    hw = [(256, 256), (128, 128), (64, 64), (32, 32)]
    hist = {}
    for roi in _bench_list(Kn, P):
        g = geom(roi, P, STRIDES)
        H, W = hw[g['level']]
        lo_x, hi_x = g['start_w'] - 1, F(g['start_w'] + F(g['bin_w'] * F(P))) + 1
        lo_y, hi_y = g['start_h'] - 1, F(g['start_h'] + F(g['bin_h'] * F(P))) + 1
        Fw = int(np.ceil(np.clip(hi_x, 0, W - 1))) - int(np.floor(np.clip(lo_x, 0, W - 1))) + 1
        Fh = int(np.ceil(np.clip(hi_y, 0, H - 1))) - int(np.floor(np.clip(lo_y, 0, H - 1))) + 1
        cb = next((c for c in (256, 128, 64) if -(-Fh * Fw // (512 // c)) * 1024 <= stage), 0)
        stream = g['bin_h'] >= 1 and g['bin_w'] >= 1
        if stream and g['count'] > gmax:
            cb = 0
        key = (K.ROI_FORM_LDS, cb) if cb else (K.ROI_FORM_WALK if stream else K.ROI_FORM_LOOP, 0)
        hist[key] = hist.get(key, 0) + 1
    return hist


@pytest.mark.parametrize('Kn,P', BENCH, ids=['bbox_8192x7', 'mask_2048x14', 'foa_2048x7'])
def test_auto_on_the_bench_lists(Kn, P):
    hist, splits = _bench_hist(Kn, P)
    assert splits == {2 if Kn <= 4096 else 1}
    assert hist == BENCH_HIST[(Kn, P)]
    assert hist == _expected_hist(Kn, P)
    assert sum(hist.values()) == Kn
    # every class of the rule occurs, so that a moved threshold moves a count
    assert {k for k in hist} >= {(K.ROI_FORM_LDS, 256), (K.ROI_FORM_LDS, 128), (K.ROI_FORM_LDS, 64), (K.ROI_FORM_WALK, 0)}, hist
    # and the thresholds are the shipped ones: another stage size or gmax gives another histogram
    assert _expected_hist(Kn, P, stage=16 * 1024) != hist and _expected_hist(Kn, P, stage=32 * 1024) != hist
    assert _expected_hist(Kn, P, gmax=3) != hist or P == 14
    assert _bench_hist(Kn, P, _T(stage_kib=24, gmax=4))[0] == hist


def test_split_rule_boundary():
    hw = [(256, 256), (128, 128), (64, 64), (32, 32)]
    for Kn, ns in ((4096, 2), (4097, 1)):
        assert K.roi_fwd_form(hw, STRIDES, 256, L.act16(), [0, 100, 100, 140, 140], Kn, 7)[5] == ns


def test_both_builds_choose_the_same_forms():
    want = [forms_of('L7', 256, L.act16()), forms_of('L14', 192, L.act16())]
    prev = L.set_act16(torch.float16)
    try:
        got = [forms_of('L7', 256, L.act16()), forms_of('L14', 192, L.act16())]
    finally:
        L.set_act16(prev)
    assert got == want
