"""BONAI sample contract on the host side of the path: annotation schema -> training sample -> device batch.

What the hot path consumes is the batch dict ``img, img_metas, gt_bboxes, gt_labels, gt_masks, gt_offsets``
(mmdet/models/detectors/two_stage.py:105-167).  This module mirrors the pieces of the reference's data pipeline that
define the *values* in that dict -- the BONAI annotation parser (mmdet/datasets/bonai.py:105-256), the flip rules for
boxes and offsets (mmdet/datasets/pipelines/transforms.py:379-404, 458-466), Normalize and DefaultFormatBundle / Collect
(pipelines/formating.py) -- and ends in ``to_device_batch``, which uploads once: images normalised on the GPU, instance
masks as uint8 device tensors (the device-side mask_target kernel crops them; no per-step CPU round trip as in
mmdet/core/mask/structures.py:261-291).  Polygon rasterisation (pycocotools in the reference) runs on the device
(kernels.poly2mask); image decoding (cv2) stays outside: it is not in this image and not on the path.
"""
import math

import numpy as np
import torch

from .kernels import D4_MIRROR_X, D4_MIRROR_Y, D4_TRANSPOSE


def parse_bonai_annotations(img_info, ann_info, cat_ids=(1,), cat2label=None, bbox_type='roof', mask_type='roof',
                            offset_coordinate='rectangle', resolution=0.6, ignore_buildings=True):
    """BONAI._parse_ann_info (bonai.py:105-256): list of COCO-style BONAI annotation dicts -> ann dict of arrays.
    Keys and dtypes follow the reference, including its empty-image conventions (angle 0.0001, heights (0, 2))."""
    cat2label = cat2label or {c: i for i, c in enumerate(cat_ids)}
    key = {'roof': 'bbox', 'building': 'building_bbox', 'footprint': 'footprint_bbox'}
    if bbox_type not in key:
        raise TypeError(f"don't support bbox_type={bbox_type}")
    if mask_type not in ('roof', 'footprint'):
        raise TypeError(f"don't support mask_type={mask_type}")
    if offset_coordinate not in ('rectangle', 'polar'):
        raise RuntimeError(f'do not support this coordinate: {offset_coordinate}')
    bboxes, labels, ignore, masks, roof_masks, fp_masks = [], [], [], [], [], []
    offsets, heights, angles, roof_bboxes, fp_bboxes = [], [], [], [], []
    only_fp = 0
    for ann in ann_info:
        if ann.get('ignore', False):
            continue
        x1, y1, w, h = ann[key[bbox_type]]
        inter_w = max(0, min(x1 + w, img_info['width']) - max(x1, 0))
        inter_h = max(0, min(y1 + h, img_info['height']) - max(y1, 0))
        if inter_w * inter_h == 0 or ann['area'] <= 0 or w < 1 or h < 1 or ann['category_id'] not in cat_ids:
            continue
        bbox = [x1, y1, x1 + w, y1 + h]
        if ann.get('iscrowd', False) and ignore_buildings:
            ignore.append(bbox)
            continue
        if 'roof_bbox' in ann:
            rx, ry, rw, rh = ann['roof_bbox']
            roof_bboxes.append([rx, ry, rx + rw, ry + rh])
        if 'footprint_bbox' in ann:
            fx, fy, fw, fh = ann['footprint_bbox']
            fp_bboxes.append([fx, fy, fx + fw, fy + fh])
        if 'only_footprint' in ann:
            only_fp = 1 if ann['only_footprint'] == 1 else 0
        bboxes.append(bbox)
        labels.append(cat2label[ann['category_id']])
        if only_fp == 0 and mask_type == 'roof':
            masks.append(ann['segmentation'])
        else:
            masks.append([ann['footprint_mask']])
        roof_masks.append(ann['segmentation'])
        fp_masks.append([ann['footprint_mask']])
        if 'offset' in ann:
            if offset_coordinate == 'rectangle':
                offsets.append(ann['offset'])
            else:
                ox, oy = ann['offset']
                offsets.append([math.sqrt(ox ** 2 + oy ** 2), math.atan2(oy, ox)])
        else:
            offsets.append([0, 0])
        heights.append(ann.get('building_height', 0.0))
        if 'offset' in ann and 'building_height' in ann:
            ox, oy = ann['offset']
            angles.append(math.atan2(math.sqrt(ox ** 2 + oy ** 2) * resolution, ann['building_height']))
    if bboxes:
        out = dict(bboxes=np.array(bboxes, dtype=np.float32), labels=np.array(labels, dtype=np.int64),
                   offsets=np.array(offsets, dtype=np.float32), building_heights=np.array(heights, dtype=np.float32),
                   angle=float(np.array(angles, dtype=np.float32).mean()) if angles else float('nan'),
                   roof_bboxes=np.array(roof_bboxes, dtype=np.float32), footprint_bboxes=np.array(fp_bboxes, dtype=np.float32),
                   only_footprint_flag=float(only_fp))
    else:
        out = dict(bboxes=np.zeros((0, 4), np.float32), labels=np.array([], dtype=np.int64), offsets=np.zeros((0, 2), np.float32),
                   building_heights=np.zeros((0, 2), np.float32), angle=0.0001, roof_bboxes=np.zeros((0, 4), np.float32),
                   footprint_bboxes=np.zeros((0, 4), np.float32), only_footprint_flag=0)
    out['bboxes_ignore'] = np.array(ignore, dtype=np.float32) if ignore else np.zeros((0, 4), np.float32)
    out.update(masks=masks, roof_masks=roof_masks, footprint_masks=fp_masks)
    fn = img_info['filename']
    out.update(seg_map=fn.replace('jpg', 'png'), edge_map=fn.replace('jpg', 'png'), side_face_map=fn.replace('jpg', 'png'),
               offset_field=fn.replace('png', 'npy'))
    return out


def flip_bboxes(bboxes, img_shape, direction):
    """RandomFlip.bbox_flip (transforms.py:379-404)."""
    out = bboxes.copy()
    if direction == 'horizontal':
        w = img_shape[1]
        out[..., 0::4] = w - bboxes[..., 2::4]
        out[..., 2::4] = w - bboxes[..., 0::4]
    elif direction == 'vertical':
        h = img_shape[0]
        out[..., 1::4] = h - bboxes[..., 3::4]
        out[..., 3::4] = h - bboxes[..., 1::4]
    else:
        raise ValueError(f"Invalid flipping direction '{direction}'")
    return out


def flip_offsets(offsets, direction):
    """RandomFlip.offset_flip (transforms.py:458-466): horizontal negates x, vertical negates y."""
    off = np.asarray(offsets, dtype=np.float32).reshape(-1, 2).copy()
    if direction == 'horizontal':
        off[:, 0] = -off[:, 0]
    elif direction == 'vertical':
        off[:, 1] = -off[:, 1]
    else:
        raise ValueError(f"Invalid flipping direction '{direction}'")
    return off


def flip_sample(sample, direction='horizontal', defer_image=False):
    """One training sample (img HxWx3, gt_bboxes, gt_masks [K,H,W] u8 -- or gt_polygons --, gt_offsets) flipped as
    RandomFlip.__call__ does (transforms.py:406-456).

    A sample that carries ``gt_polygons`` instead of bitmaps keeps its polygons as they are and records the flip in
    ``mask_flips``: the reference's pipeline rasterises first (LoadAnnotations(poly2mask=True), loading.py:301-326 ->
    BitmapMasks) and RandomFlip then mirrors the BITMAP (structures.py:218-229), which is not the same pixels as rasterising
    mirrored vertices (pycocotools' edge walk is not flip-symmetric); ``to_device_batch`` rasterises on the device and
    mirrors the bitmap there, in the recorded order -- bit-identical to the host bitmap path."""
    if direction not in ('horizontal', 'vertical'):
        raise ValueError(f"Invalid flipping direction '{direction}'")
    h, w = _frame(sample)
    ax = 1 if direction == 'horizontal' else 0
    out = dict(sample)
    _resized_needs_deferral(sample, defer_image)
    if defer_image:          # the prefetching loader: the image is mirrored on the device after the upload (to_device_batch)
        out['img_flip'] = tuple(sample.get('img_flip', ())) + (direction,)
    else:
        out['img'] = np.flip(sample['img'], axis=ax).copy()
    out['gt_bboxes'] = flip_bboxes(sample['gt_bboxes'], (h, w), direction)
    if sample.get('gt_masks') is not None:
        out['gt_masks'] = np.flip(sample['gt_masks'], axis=ax + 1).copy()
    elif 'gt_polygons' in sample:
        out['mask_flips'] = tuple(sample.get('mask_flips', ())) + (direction,)
    else:
        raise KeyError("flip_sample: the sample carries neither 'gt_masks' nor 'gt_polygons'")
    out['gt_offsets'] = flip_offsets(sample['gt_offsets'], direction)
    out['flip'], out['flip_direction'] = True, direction
    return out


# ---- Resize (transforms.py:34-349) and Pad (:560-640) ----------------------------------------------------------------------------
# The sample-level algebra only: sizes, scale draws, boxes, offsets, meta.  The pixels are resampled on the device, after the upload
# (kernels.image_resize_prep / mask_resize_u8), so a resized sample keeps its SOURCE image and carries the geometry in 'resize'.


def rescale_size(old_size, scale):
    """mmcv.imrescale's size rule for a tuple scale, from memory of mmcv/image/geometric.py (mmcv is not installed where this
    was written): (w, h), (a, b) -> (new_w, new_h) with s = min(long / max(h, w), short / min(h, w)) and int(x * s + 0.5)."""
    w, h = old_size
    long_edge, short_edge = max(scale), min(scale)
    s = min(long_edge / max(h, w), short_edge / min(h, w))
    return int(w * float(s) + 0.5), int(h * float(s) + 0.5)


def random_select(img_scales, rng):
    """Resize.random_select (transforms.py:87-102)."""
    return img_scales[rng.randint(len(img_scales))]


def random_sample(img_scales, rng):
    """Resize.random_sample (transforms.py:105-129): the long edge is drawn first, then the short edge."""
    if len(img_scales) != 2:
        raise ValueError(f"multiscale_mode='range' takes two scales, got {img_scales}")
    longs, shorts = [max(s) for s in img_scales], [min(s) for s in img_scales]
    long_edge = rng.randint(min(longs), max(longs) + 1)
    short_edge = rng.randint(min(shorts), max(shorts) + 1)
    return int(long_edge), int(short_edge)


def random_sample_ratio(img_scale, ratio_range, rng):
    """Resize.random_sample_ratio (transforms.py:132-156)."""
    min_ratio, max_ratio = ratio_range
    if not min_ratio <= max_ratio:
        raise ValueError(f'ratio_range {ratio_range}: the minimum comes first')
    ratio = rng.random_sample() * (max_ratio - min_ratio) + min_ratio
    return int(img_scale[0] * ratio), int(img_scale[1] * ratio)


def random_scale(img_scales, multiscale_mode, ratio_range, rng):
    """Resize._random_scale (transforms.py:158-189).  A single scale without a ratio_range draws nothing."""
    if ratio_range is not None:
        return random_sample_ratio(img_scales[0], ratio_range, rng)
    if len(img_scales) == 1:
        return tuple(img_scales[0])
    if multiscale_mode == 'range':
        return random_sample(img_scales, rng)
    if multiscale_mode == 'value':
        return tuple(random_select(img_scales, rng))
    raise NotImplementedError(f'multiscale_mode={multiscale_mode!r}')


def resize_geometry(src_shape, scale, keep_ratio=True, pad_divisor=32):
    """Resize._resize_img's bookkeeping (transforms.py:191-220) and Pad's (:590-600) for a source of src_shape = (h, w):
    -> dict(size=(new_h, new_w), pad=(pad_h, pad_w), w_scale, h_scale).  keep_ratio=False is mmcv.imresize: scale is (w, h)."""
    h, w = src_shape[:2]
    new_w, new_h = rescale_size((w, h), scale) if keep_ratio else (int(scale[0]), int(scale[1]))
    if new_w < 1 or new_h < 1:
        raise ValueError(f'scale {scale} resizes a {w}x{h} image to {new_w}x{new_h}')
    d = int(pad_divisor) if pad_divisor else 1
    pad = (int(np.ceil(new_h / d)) * d, int(np.ceil(new_w / d)) * d)
    return dict(size=(new_h, new_w), pad=pad, w_scale=new_w / w, h_scale=new_h / h, keep_ratio=bool(keep_ratio))


def resize_sample(sample, scale, keep_ratio=True, pad_divisor=32):
    """One training sample under Resize(scale, keep_ratio) followed, at the end of the pipeline, by Pad(size_divisor).  Boxes are
    multiplied by the float32 scale_factor and clipped to img_shape (_resize_bboxes, transforms.py:222-229).  The image and the
    bitmaps stay at the source size: 'resize' carries the geometry to ``to_device_batch``.

    DEVIATION: the reference's Resize.__call__ (transforms.py:334-341) never touches ``offset_fields``, so at any scale other
    than 1 its gt_offsets are not in the resized image's frame.  Here they are multiplied by (w_scale, h_scale)."""
    if sample.get('gt_masks') is not None:
        raise NotImplementedError('Resize takes polygon samples (gt_polygons): the bitmaps are rasterised at the source size and '
                                  'resized on the device')
    if 'resize' in sample or sample.get('img_flip') or sample.get('flip') or sample.get('rotate'):
        raise ValueError('Resize comes first in the pipeline: the sample has been resized, flipped or rotated already')
    g = resize_geometry(sample['img'].shape, scale, keep_ratio, pad_divisor)
    factor = np.array([g['w_scale'], g['h_scale'], g['w_scale'], g['h_scale']], dtype=np.float32)
    out = dict(sample)
    bboxes = np.asarray(sample['gt_bboxes'], np.float32).reshape(-1, 4) * factor
    bboxes[:, 0::2] = np.clip(bboxes[:, 0::2], 0, g['size'][1])
    bboxes[:, 1::2] = np.clip(bboxes[:, 1::2], 0, g['size'][0])
    out['gt_bboxes'] = bboxes
    out['gt_offsets'] = np.asarray(sample['gt_offsets'], np.float32).reshape(-1, 2) * factor[:2]
    out['resize'] = g
    out['img_shape'] = g['size'] + (3,)
    out['scale_factor'] = factor
    return out


def _frame(sample):
    """(h, w) of the frame the sample's boxes live in: the resized image's for a resized sample, else the image's own."""
    return tuple(sample['img_shape'][:2]) if 'resize' in sample else sample['img'].shape[:2]


def _resized_needs_deferral(sample, defer_image):
    if 'resize' in sample and not defer_image:
        raise ValueError('a resized sample keeps its source pixels: flips and rotations of it are deferred to the device '
                         '(defer_image=True)')


RIGHT_ANGLES = (0, 90, 180, 270)
_WHY_RIGHT_ANGLES = (
    'RandomRotate is supported for the angles 0, 90, 180 and 270 only (got {got}).  For any other angle the reference has '
    'nothing sound to mirror: its bbox_rotate (transforms.py:1975-2014) shifts the boxes by (nW/2 - cx, nH/2 - cy), the offset of '
    'an EXPANDED canvas, while the image is rotated with auto_bound=False and is not expanded -- the boxes do not lie on the '
    "reference's own image (212 px off at 45 degrees on a 1024 tile).  choice='any' (a string: range(0, 359)) is such a choice.")


def check_rotate_angles(angles):
    """The angles of a RandomRotate ``choice`` as a tuple of ints; NotImplementedError (with the reason) unless every one of them
    is a right angle.  A string is the reference's 'any' (transforms.py:1853-1854)."""
    if isinstance(angles, str) or not isinstance(angles, (list, tuple)):
        raise NotImplementedError(_WHY_RIGHT_ANGLES.format(got=repr(angles)))
    for a in angles:
        if isinstance(a, (bool, str)) or a not in RIGHT_ANGLES:
            raise NotImplementedError(_WHY_RIGHT_ANGLES.format(got=repr(tuple(angles))))
    return tuple(int(a) for a in angles)


def _rotation_matrix(center, angle, scale=1.0):
    """cv2.getRotationMatrix2D from OpenCV's documented formula (cv2 is not a dependency): with a = scale * cos(angle) and
    b = scale * sin(angle), angle in degrees, [[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]] in float64."""
    rad = angle * math.pi / 180.0
    a, b = scale * math.cos(rad), scale * math.sin(rad)
    cx, cy = center
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=np.float64)


def rotate_bboxes(bboxes, img_shape, angle):
    """RandomRotate.bbox_rotate (transforms.py:1975-2014), get_corners (:1862-1898) included: the four corners of every box (the
    second and third rebuilt from x1 + width, y1 + height in the boxes' own dtype, as there), times the float64 matrix about
    (w / 2, h / 2) with -angle, cast to float32, then min / max per box.

    The reference's half-pixel quirk is kept and is consistent: boxes are in pixel-EDGE coordinates, so turning them about
    w / 2 is turning the pixel centres about (w - 1) / 2, which is what mmcv.imrotate does to the image.  The reference also
    re-centres on an expanded canvas (nW, nH) although the image is not expanded; for the supported angles on a square tile
    nW == w and nH == h and the shift is zero (see ``check_rotate_angles`` for the others)."""
    angle, = check_rotate_angles((angle,))
    bboxes = np.asarray(bboxes)
    assert bboxes.shape[-1] % 4 == 0
    if bboxes.shape[0] == 0:
        return bboxes
    h, w = img_shape[:2]
    if angle in (90, 270) and h != w:
        raise NotImplementedError(f'RandomRotate by {angle} needs a square tile, got {w}x{h}: the rotated image is not expanded')
    x1, y1 = bboxes[:, 0].reshape(-1, 1), bboxes[:, 1].reshape(-1, 1)
    width, height = (bboxes[:, 2] - bboxes[:, 0]).reshape(-1, 1), (bboxes[:, 3] - bboxes[:, 1]).reshape(-1, 1)
    corners = np.hstack((x1, y1, x1 + width, y1, x1, y1 + height, bboxes[:, 2].reshape(-1, 1), bboxes[:, 3].reshape(-1, 1)))
    corners = np.hstack((corners, bboxes[:, 4:])).reshape(-1, 2)
    corners = np.hstack((corners, np.ones((corners.shape[0], 1), dtype=corners.dtype)))
    cx, cy = w / 2, h / 2
    M = _rotation_matrix((cx, cy), -angle, 1.0)
    cos, sin = np.abs(M[0, 0]), np.abs(M[0, 1])
    M[0, 2] += int(h * sin + w * cos) / 2 - cx
    M[1, 2] += int(h * cos + w * sin) / 2 - cy
    calc = np.array(np.dot(M, corners.T).T, dtype=np.float32).reshape(-1, 8)
    xs, ys = calc[:, [0, 2, 4, 6]], calc[:, [1, 3, 5, 7]]
    return np.hstack((xs.min(1).reshape(-1, 1), ys.min(1).reshape(-1, 1), xs.max(1).reshape(-1, 1), ys.max(1).reshape(-1, 1)))


def rotate_offsets(offsets, angle):
    """RandomRotate.offset_rotate (transforms.py:1957-1964): per offset a polar round trip -- length = math.sqrt(x**2 + y**2) and
    math.atan2(y, x) on the float32 elements, the angle plus angle * pi / 180, length * np.cos / np.sin in float64 -- then the
    float32 cast.  Deliberately NOT a sign swap: cos(pi / 2) is 6e-17, and what of 6e-17 * length survives the cast survives
    here as it does there (a rotated (0, y) has x = 6e-17 * y, not 0)."""
    angle, = check_rotate_angles((angle,))
    out = []
    for ox, oy in np.asarray(offsets, dtype=np.float32).reshape(-1, 2):
        length, phi = math.sqrt(ox ** 2 + oy ** 2), math.atan2(oy, ox) + angle * math.pi / 180.0
        out.append([length * np.cos(phi), length * np.sin(phi)])
    return np.array(out, dtype=np.float32).reshape(-1, 2)


# ---- the eight symmetries of the square ------------------------------------------------------------------------------------------
# RandomFlip and right-angle RandomRotate, in any order and number, compose to ONE element: an optional transpose, then an optional
# x-mirror, then an optional y-mirror (include/loft_hip.h LOFT_D4_*: 1, 2, 4).  The rule for the angle: mmcv.imrotate(img, angle,
# auto_bound=False) turns about ((w - 1) / 2, (h - 1) / 2) with cv2.getRotationMatrix2D(center, -angle, 1); from OpenCV's
# documented matrix, source pixel (x, y) lands at (S-1-y, x) for 90, (S-1-x, S-1-y) for 180, (y, S-1-x) for 270 -- an exact
# pixel permutation, np.rot90(a, k=-angle // 90): clockwise for a positive angle.  cv2 and mmcv are not installed where this was
# written, so that equality is DERIVED from the documentation and has not been run against them.


def d4_apply(a, elem, axes=(0, 1)):
    """numpy view of ``a`` under an element, rows = axes[0], columns = axes[1] (the definition the kernels are tested against)."""
    ay, ax = axes
    if elem & D4_TRANSPOSE:
        a = np.swapaxes(a, ay, ax)
    if elem & D4_MIRROR_X:
        a = np.flip(a, ax)
    if elem & D4_MIRROR_Y:
        a = np.flip(a, ay)
    return a


def _d4_op(a, op, axes=(0, 1)):
    """One recorded operation -- 'horizontal', 'vertical' or a right angle -- on a numpy array."""
    if op == 'horizontal':
        return np.flip(a, axes[1])
    if op == 'vertical':
        return np.flip(a, axes[0])
    if isinstance(op, str):
        raise ValueError(f"Invalid flipping direction '{op}'")
    angle, = check_rotate_angles((op,))
    return np.rot90(a, k=-angle // 90, axes=axes)


_D4_PROBE = np.arange(4).reshape(2, 2)
_D4_OF = {d4_apply(_D4_PROBE, e).tobytes(): e for e in range(8)}      # a 2 x 2 array tells the eight elements apart


def d4_compose(ops):
    """The ordered record of flips and right-angle rotations (what ``img_flip`` / ``mask_flips`` hold) -> the one element that
    does the same.  Flips and rotations do not commute; the record is applied to a 2 x 2 probe in order and looked up."""
    p = _D4_PROBE
    for op in ops:
        p = _d4_op(p, op)
    return _D4_OF[np.ascontiguousarray(p).tobytes()]


def _carries_rotation(ops):
    return any(not isinstance(op, str) for op in ops)


def rotate_sample(sample, angle, defer_image=False):
    """One training sample rotated as RandomRotate.__call__ does (transforms.py:2016-2092), for a right angle on a square tile
    (``check_rotate_angles`` says why no other).  Shaped like ``flip_sample``: host bitmaps are turned with np.rot90; a sample
    that carries ``gt_polygons`` records the angle in ``mask_flips`` -- the reference rasterises first and permutes the BITMAP,
    and so does ``to_device_batch`` --; ``defer_image`` records it in ``img_flip`` for the device.  The record is ordered: a
    flip before a rotation is not the rotation before the flip.

    Angle 0 with rotate=True leaves the pixels alone (nothing is recorded) but, as in the reference, still sends boxes and
    offsets through bbox_rotate / offset_rotate, and ``rotate`` stays True in the meta."""
    angle, = check_rotate_angles((angle,))
    h, w = _frame(sample)
    if angle in (90, 270) and h != w:
        raise NotImplementedError(f'RandomRotate by {angle} needs a square tile, got {w}x{h}: the rotated image is not expanded')
    k = -angle // 90
    out = dict(sample)
    _resized_needs_deferral(sample, defer_image)
    if angle:
        if defer_image:
            out['img_flip'] = tuple(sample.get('img_flip', ())) + (angle,)
        else:
            out['img'] = np.ascontiguousarray(np.rot90(sample['img'], k=k, axes=(0, 1)))
    out['gt_bboxes'] = rotate_bboxes(sample['gt_bboxes'], (h, w, 3), angle)
    if sample.get('gt_masks') is not None:
        if angle:
            out['gt_masks'] = np.ascontiguousarray(np.rot90(sample['gt_masks'], k=k, axes=(1, 2)))
    elif 'gt_polygons' in sample:
        if angle:
            out['mask_flips'] = tuple(sample.get('mask_flips', ())) + (angle,)
    else:
        raise KeyError("rotate_sample: the sample carries neither 'gt_masks' nor 'gt_polygons'")
    out['gt_offsets'] = rotate_offsets(sample['gt_offsets'], angle)
    out['rotate'], out['rotate_angle'] = True, angle
    return out


def _permute_masks(m, ops, resize=None):
    """Rasterised bitmaps [K,H,W] of a polygon sample under its recorded operations.  Flips alone: the mirrored copies as before;
    a record with a rotation: composed to one element, one launch of loft_mask_d4_u8.  A resized sample (``resize``: its
    geometry): nearest-neighbour Resize, the element and Pad in one launch of loft_mask_resize_d4_u8."""
    if resize is not None:
        from . import kernels as K
        return K.mask_resize_u8(m.contiguous(), resize['size'], resize['pad'], d4_compose(ops))
    if not _carries_rotation(ops):
        for d in ops:                                       # flip_sample on a polygon sample: the bitmap is mirrored, as the
            m = m.flip(2 if d == 'horizontal' else 1)       # reference's RandomFlip does after LoadAnnotations rasterised it
        return m.contiguous()
    elem = d4_compose(ops)
    if elem == 0 or m.shape[0] == 0:
        return m.contiguous()
    from . import kernels as K
    return K.mask_d4(m.contiguous(), elem)


def _masks_of(s, dev):
    if 'gt_polygons' in s and s.get('gt_masks') is None:
        from . import kernels as K
        h, w = s['img'].shape[:2]
        m = K.poly2mask(s.get('gt_polygons_packed') or s['gt_polygons'], h, w, device=dev)
        return _permute_masks(m, s.get('mask_flips', ()), s.get('resize'))
    if 'resize' in s:
        raise NotImplementedError('Resize takes polygon samples (gt_polygons), not host bitmaps')
    return torch.from_numpy(np.ascontiguousarray(s['gt_masks'], dtype=np.uint8)).to(dev)


def _normalise_torch(imgs, rgb, flips, mean, std, to_rgb, dev):
    """Normalize + bundle of a batch that carries no rotation: uint8 / float [n,H,W,3] -> fp32 [n,3,H,W]; ``flips``: per sample the
    deferred RandomFlip directions."""
    x = imgs.float()
    if to_rgb and not all(rgb):
        if any(rgb):
            keep = torch.tensor(rgb, device=dev).view(-1, 1, 1, 1)
            x = torch.where(keep, x, x.flip(-1))
        else:
            x = x.flip(-1)
    for i, dirs in enumerate(flips):                                 # RandomFlip's image mirror, deferred by the loader
        for d in dirs:
            x[i] = x[i].flip(1 if d == 'horizontal' else 0)
    x = (x - torch.tensor(mean, device=dev)) / torch.tensor(std, device=dev)
    return x.permute(0, 3, 1, 2).contiguous()


def to_device_batch(samples, device='cuda', mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), to_rgb=True, staged=None):
    """Collate + DefaultFormatBundle + Normalize, on the device: list of samples (img uint8/float HxWx3 BGR, gt_* numpy) ->
    the batch dict of forward_train.  Images are stacked (same size: BONAI tiles are 1024x1024), normalised on the GPU;
    ``staged``: the images as one uint8 [n,H,W,3] host tensor (BonaiDataset's pinned staging ring; sample['img'] are views of it).
    masks go up once as uint8 [K,H,W] tensors -- or, when a sample carries ``gt_polygons`` (per instance a list of flat polygons: the
    annotation's ``masks`` entry, bonai.py:186-199) instead of ``gt_masks``, only the vertices go up and the bitmaps are rasterised on the
    device (kernels.poly2mask = LoadAnnotations._poly2mask, loading.py:301-326): no K x 1024^2 host bitmaps, no upload.
    A batch in which some sample's deferred record (``img_flip``) holds a rotation is normalised by kernels.image_prep_d4, and that
    sample's rasterised bitmaps are permuted by kernels.mask_d4; a batch without a rotation takes the torch chain as before."""
    dev = torch.device(device)
    if staged is not None:       # uint8 [n, H, W, 3] holding the samples' images already (a pinned staging slot): one async upload
        imgs = staged.to(dev, non_blocking=True)
    else:
        imgs = torch.stack([torch.from_numpy(np.ascontiguousarray(s['img'])) for s in samples]).to(dev)
    rgb = [bool(s.get('img_rgb', False)) for s in samples]         # decoded straight to RGB: Normalize's reversal already done
    if not to_rgb and any(rgb):
        raise ValueError('samples decoded to RGB need to_rgb=True (the configured Normalize of bonai_instance.py:3-4)')
    geoms = [s.get('resize') for s in samples]
    if any(g is not None for g in geoms):
        # Resize (and Pad): one geometry per batch -- loft_rpn_decode takes one img_shape per batch -- and the whole chain,
        # Resize, the element of the deferred record, channel order, Normalize, Pad, HWC -> CHW, in one launch
        if any(g != geoms[0] for g in geoms):
            raise NotImplementedError('a batch takes ONE scale (per-sample scale draws are not supported): its samples carry '
                                      f'{sorted({(g["size"], g["pad"]) if g else None for g in geoms}, key=str)}')
        from . import kernels as K
        img = K.image_resize_prep(imgs, geoms[0]['size'], geoms[0]['pad'], [d4_compose(s.get('img_flip', ())) for s in samples],
                                  [r or not to_rgb for r in rgb], mean, std)
    elif any(_carries_rotation(s.get('img_flip', ())) for s in samples):
        # RandomRotate's image permutation, deferred by the loader: every sample's record of flips and rotations composed to one
        # element, and the whole batch -- permutation, channel order, Normalize, HWC -> CHW -- in one launch
        elems = [d4_compose(s.get('img_flip', ())) for s in samples]
        if dev.type == 'cuda':
            from . import kernels as K
            img = K.image_prep_d4(imgs, elems, [r or not to_rgb for r in rgb], mean, std)
        else:             # host tensors (device='cpu': the loader's CPU tests): the same permutation on the uint8 tiles, with numpy
            imgs = torch.stack([torch.from_numpy(np.ascontiguousarray(d4_apply(t.numpy(), e))) for t, e in zip(imgs, elems)])
            img = _normalise_torch(imgs, rgb, [()] * len(samples), mean, std, to_rgb, dev)
    else:
        img = _normalise_torch(imgs, rgb, [s.get('img_flip', ()) for s in samples], mean, std, to_rgb, dev)
    metas = []
    for s in samples:
        h, w = s['img'].shape[:2]
        metas.append(dict(filename=s.get('filename'), ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(h, w, 3),
                          scale_factor=np.array([1., 1., 1., 1.], dtype=np.float32), flip=bool(s.get('flip', False)),
                          flip_direction=s.get('flip_direction'), rotate=bool(s.get('rotate', False)),
                          rotate_angle=int(s.get('rotate_angle', 0)),
                          img_norm_cfg=dict(mean=np.array(mean, np.float32), std=np.array(std, np.float32), to_rgb=to_rgb)))
        if 'resize' in s:                   # Resize's and Pad's entries (transforms.py:216-220, 597-599)
            g = s['resize']
            metas[-1].update(img_shape=g['size'] + (3,), pad_shape=g['pad'] + (3,), scale_factor=s['scale_factor'],
                             keep_ratio=g['keep_ratio'])
    if dev.type == 'cuda' and staged is not None:
        # the loader's path: every small array of the batch (boxes, labels, offsets, polygon vertices and their offset tables)
        # in ONE pinned buffer and ONE asynchronous copy -- 48 pageable synchronous copies of a few hundred bytes each were
        # 5 of the 6 ms this function held the interpreter lock next to the training loop
        return dict(img=img, img_metas=metas, **_small_arrays_one_copy(samples, dev))
    return dict(img=img, img_metas=metas,
                gt_bboxes=[torch.from_numpy(np.asarray(s['gt_bboxes'], np.float32)).to(dev) for s in samples],
                gt_labels=[torch.from_numpy(np.asarray(s['gt_labels'], np.int64)).to(dev) for s in samples],
                gt_masks=[_masks_of(s, dev) for s in samples],
                gt_offsets=[torch.from_numpy(np.asarray(s['gt_offsets'], np.float32).reshape(-1, 2)).to(dev) for s in samples])


def _small_arrays_one_copy(samples, dev):
    from . import kernels as K
    arrs, slots = [], []          # (numpy array) and (sample index, field)
    packs = []
    for i, s in enumerate(samples):
        arrs += [np.ascontiguousarray(s['gt_bboxes'], np.float32), np.ascontiguousarray(s['gt_labels'], np.int64),
                 np.ascontiguousarray(np.asarray(s['gt_offsets'], np.float32).reshape(-1, 2))]
        slots += [(i, 'gt_bboxes'), (i, 'gt_labels'), (i, 'gt_offsets')]
        pk = None
        if 'gt_polygons' in s and s.get('gt_masks') is None:
            pk = s.get('gt_polygons_packed') or K.pack_polygons(s['gt_polygons'])
            arrs += [pk.xy, pk.poff, pk.ioff]
            slots += [(i, '_xy'), (i, '_poff'), (i, '_ioff')]
        packs.append(pk)
    offs, total = [], 0
    for a in arrs:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for a, o in zip(arrs, offs):
        if a.nbytes:
            hv[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    devb = host.to(dev, non_blocking=True)
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64}
    out = dict(gt_bboxes=[None] * len(samples), gt_labels=[None] * len(samples), gt_offsets=[None] * len(samples))
    aux = [dict() for _ in samples]
    for a, o, (i, name) in zip(arrs, offs, slots):
        t = devb[o:o + a.nbytes].view(tdt[a.dtype]).view(a.shape)
        if name[0] == '_':
            aux[i][name] = t
        else:
            out[name][i] = t
    masks = []
    for i, s in enumerate(samples):
        if packs[i] is None:
            masks.append(_masks_of(s, dev))
            continue
        h, w = s['img'].shape[:2]
        m = K.poly2mask_device(aux[i]['_xy'], aux[i]['_poff'], aux[i]['_ioff'], packs[i].n, h, w, packs[i].maxv)
        masks.append(_permute_masks(m, s.get('mask_flips', ()), s.get('resize')))
    out['gt_masks'] = masks
    return out
