"""Test-time augmentation: the views of a tile and their algebra (host side; the merges are bonai_amd/csrc/tta.hip).

A view is one operation on the tile -- ``None`` (the tile itself), ``'horizontal'`` / ``'vertical'`` (the reference's
MultiScaleFlipAug flips, mmdet/datasets/pipelines/test_time_aug.py:10-82) or a right angle 90 / 180 / 270 (an extension, like the
right-angle-only RandomRotate) -- and stands for one element of the square's symmetry group in the D4_TRANSPOSE | D4_MIRROR_X |
D4_MIRROR_Y encoding of kernels.image_prep_d4 (data.d4_compose).  A view list always starts with the tile itself.

What mirrors the reference: the view order of MultiScaleFlipAug (unflipped, then one view per flip direction) and, in the heads,
merged proposals, boxes, scores and masks for flip views.  Extensions: rotation views, and merged offsets (the reference's
StandardRoIHead.aug_test returns no offsets at all).
"""
import numpy as np

from .data import check_rotate_angles, d4_compose
from .kernels import D4_MIRROR_X, D4_MIRROR_Y, D4_TRANSPOSE

META_KEY = 'd4_element'        # img_meta key: the view's composed element
_CLI = {'h': 'horizontal', 'v': 'vertical', 'r90': 90, 'r180': 180, 'r270': 270}


def view_element(op):
    """One view operation -> its element."""
    return 0 if op is None else d4_compose([op])


def d4_inverse(elem):
    """The element that undoes ``elem``.  Mirrors and the plain transpose are their own inverses; with a transpose, undoing
    'transpose, x-mirror, y-mirror' is 'y-mirror, x-mirror, transpose' = 'transpose, then the mirrors with x and y exchanged'."""
    if not elem & D4_TRANSPOSE:
        return elem
    return D4_TRANSPOSE | (D4_MIRROR_X if elem & D4_MIRROR_Y else 0) | (D4_MIRROR_Y if elem & D4_MIRROR_X else 0)


def make_views(flip_directions=(), rotate_angles=(), tile=None):
    """-> the view list [None, flips in the order given, then rotations].  ``tile``: (h, w); 90 / 270 on a non-square tile raises the
    way RandomRotate does."""
    if isinstance(flip_directions, str):
        flip_directions = [flip_directions]
    views = [None]
    for d in flip_directions or ():
        if d not in ('horizontal', 'vertical'):
            raise ValueError(f"Invalid flipping direction '{d}'")
        views.append(d)
    for a in check_rotate_angles(tuple(rotate_angles or ())):
        if a == 0:
            raise ValueError('rotate_angles: 0 is the unrotated view, which a view list always starts with')
        if tile is not None and a in (90, 270) and tile[0] != tile[1]:
            raise NotImplementedError(f'a test view rotated by {a} needs a square tile, got {tile[1]}x{tile[0]}: the rotated image is '
                                      'not expanded')
        views.append(a)
    if len(set(view_element(v) for v in views)) != len(views):
        raise ValueError(f'test views {views}: the same symmetry twice')
    return views


def parse_tta_arg(text, tile=None):
    """tools/test.py --tta: 'h,v,r90,r180,r270' (any subset, flips first as in the config) -> view list."""
    names = [t.strip() for t in text.split(',') if t.strip()]
    bad = [t for t in names if t not in _CLI]
    if bad:
        raise ValueError(f'--tta takes a comma-separated subset of {sorted(_CLI)}, got {bad}')
    ops = [_CLI[t] for t in names]
    return make_views([o for o in ops if isinstance(o, str)], [o for o in ops if not isinstance(o, str)], tile)


def views_from_pipeline(pipeline, tile=(1024, 1024)):
    """cfg.data.test.pipeline -> view list, or None when the pipeline asks for no augmentation (flip=False and no rotate_angles:
    nothing changes).  More than one scale, or a scale other than the dataset tile, raises: the device path takes fixed-size tiles."""
    aug = [p for p in (pipeline or ()) if p.get('type') == 'MultiScaleFlipAug']
    if not aug:
        return None
    aug = aug[0]
    flip, angles = bool(aug.get('flip', False)), tuple(aug.get('rotate_angles', ()) or ())
    if not flip and not angles:
        return None
    scale = aug.get('img_scale')
    if isinstance(scale, list):
        if len(scale) != 1:
            raise NotImplementedError(f'MultiScaleFlipAug img_scale={scale}: multi-scale test views are not supported')
        scale = scale[0]
    if scale is not None and tuple(scale) != (tile[1], tile[0]) and tuple(scale) != tuple(tile):
        raise NotImplementedError(f'MultiScaleFlipAug img_scale={scale} is not the dataset tile {tile}: resized test views are not '
                                  'supported')
    factor = aug.get('scale_factor')
    if factor is not None and (isinstance(factor, (list, tuple)) and len(factor) != 1 or
                               float(np.asarray(factor).reshape(-1)[0]) != 1.0):
        raise NotImplementedError(f'MultiScaleFlipAug scale_factor={factor}: resized or multi-scale test views are not supported')
    dirs = aug.get('flip_direction', 'horizontal') if flip else ()
    return make_views(dirs, angles, tile)


def resize_from_pipeline(pipeline, tile=(1024, 1024)):
    """cfg.data.test.pipeline -> BonaiDataset's ``resize`` / ``pad_divisor`` arguments when its MultiScaleFlipAug entry resizes the
    dataset's tiles (``tile`` = (h, w)): flip=False and a single img_scale other than the tile.  None: the tiles are taken as they
    are.  More than one scale, a scale_factor, or a resized view together with flips or rotations raises."""
    aug = next((p for p in (pipeline or ()) if p.get('type') == 'MultiScaleFlipAug'), None)
    if aug is None:
        return None
    scale, factor = aug.get('img_scale'), aug.get('scale_factor')
    scales = list(scale) if isinstance(scale, list) else [] if scale is None else [scale]
    factors = list(factor) if isinstance(factor, (list, tuple)) else [] if factor is None else [factor]
    if len(scales) > 1 or len(factors) > 1:
        raise NotImplementedError(f'MultiScaleFlipAug img_scale={scale} scale_factor={factor}: multi-scale test views are not supported')
    if factors and float(factors[0]) != 1.0:
        raise NotImplementedError(f'MultiScaleFlipAug scale_factor={factor}: give the resized size as img_scale')
    inner = aug.get('transforms') or ()
    divisor = next((p.get('size_divisor') for p in inner if p.get('type') == 'Pad'), None)
    keep_ratio = next((p.get('keep_ratio', True) for p in inner if p.get('type') == 'Resize'), True)
    fits = not divisor or not (tile[0] % divisor or tile[1] % divisor)
    if (not scales or (tuple(scales[0]) in (tuple(tile), tuple(tile)[::-1]) and keep_ratio)) and fits:
        return None
    if aug.get('flip', False) or aug.get('rotate_angles'):
        raise NotImplementedError('a resized test view together with flips or rotations is not supported')
    return dict(resize=dict(img_scale=tuple(scales[0]) if scales else tuple(tile)[::-1], keep_ratio=keep_ratio), pad_divisor=divisor)


def view_meta(meta, op):
    """The img_meta of one view: the tile's meta with flip / flip_direction / rotate / rotate_angle as the train loader records
    them, the composed element under META_KEY, and the view's own img_shape."""
    m = dict(meta)
    e = view_element(op)
    m.update(flip=isinstance(op, str), flip_direction=op if isinstance(op, str) else None,
             rotate=op is not None and not isinstance(op, str), rotate_angle=0 if op is None or isinstance(op, str) else int(op))
    m[META_KEY] = e
    if e & D4_TRANSPOSE:
        for k in ('img_shape', 'pad_shape'):
            h, w = meta[k][:2]
            m[k] = (w, h) + tuple(meta[k][2:])
    return m


def meta_element(meta):
    """The element of a view's img_meta (composed from the flip / rotate record when the key is absent: a hand-built meta)."""
    if META_KEY in meta:
        return int(meta[META_KEY])
    ops = ([meta['flip_direction'] or 'horizontal'] if meta.get('flip') else []) + \
          ([int(meta['rotate_angle'])] if meta.get('rotate') and meta.get('rotate_angle') else [])
    return d4_compose(ops)


# ---- numpy statement of the maps (what the kernels and the tests' restatement are checked against) --------------------------------
def map_boxes(boxes, elem, img_shape, back=False):
    """boxes [..., 4k] float32 into the view ``elem`` of an img_shape = (h, w) tile, or back from it: transpose, x-mirror, y-mirror in
    that order (reverse order back); a mirror is bbox_flip's x1' = W - x2, x2' = W - x1 in float32."""
    b = np.array(boxes, dtype=np.float32, copy=True)
    h, w = img_shape[:2]
    hv, wv = (w, h) if elem & D4_TRANSPOSE else (h, w)

    def transpose(a):
        out = a.copy()
        out[..., 0::2], out[..., 1::2] = a[..., 1::2], a[..., 0::2]
        return out

    def mirror(a, lo, size):
        out = a.copy()
        out[..., lo::4] = np.float32(size) - a[..., lo + 2::4]
        out[..., lo + 2::4] = np.float32(size) - a[..., lo::4]
        return out
    steps = []
    if elem & D4_TRANSPOSE:
        steps.append(transpose)
    if elem & D4_MIRROR_X:
        steps.append(lambda a: mirror(a, 0, wv))
    if elem & D4_MIRROR_Y:
        steps.append(lambda a: mirror(a, 1, hv))
    for f in (reversed(steps) if back else steps):
        b = f(b)
    return b


def map_offsets(offsets, elem, back=False):
    """offset vectors [n, 2] into the view or back: a transpose swaps the components, an x-mirror negates x, a y-mirror negates y."""
    o = np.array(offsets, dtype=np.float32, copy=True).reshape(-1, 2)
    steps = []
    if elem & D4_TRANSPOSE:
        steps.append(lambda a: a[:, ::-1].copy())
    if elem & D4_MIRROR_X:
        steps.append(lambda a: a * np.array([-1, 1], np.float32))
    if elem & D4_MIRROR_Y:
        steps.append(lambda a: a * np.array([1, -1], np.float32))
    for f in (reversed(steps) if back else steps):
        o = f(o)
    return o
