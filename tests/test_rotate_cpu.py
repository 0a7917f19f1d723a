"""CPU: RandomRotate by right angles (mmdet/datasets/pipelines/transforms.py:1837-2096) on the host side -- the box and offset rules
against values recorded from the reference's own bbox_rotate / offset_rotate (tests/golden/random_rotate.npz, written by
tools/make_rotate_goldens.py), the direction of image, bitmaps, boxes and offsets tied together on small bitmaps, the composition
with RandomFlip, the random stream of the loaders, and the configuration surface."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from bonai_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = (0, 90, 180, 270)


@pytest.fixture(scope='module')
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'random_rotate.npz'))
    return {k: g[k] for k in g.files}


def _ulps(a, b):
    """Distance in float32 units in the last place of the larger magnitude (0 for equal values, signed zeros included)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


def test_rotate_bboxes_equals_the_reference(golden):
    assert tuple(golden['angles']) == ANGLES and golden['bboxes'].shape[0] >= 16
    b = golden['bboxes']
    assert (b[:, 0] == 0).any() and (b[:, 2] == 1024).any() and ((b[:, 0] == b[:, 2]) & (b[:, 1] == b[:, 3])).any()
    for a in ANGLES:
        got = D.rotate_bboxes(golden['bboxes'], tuple(golden['img_shape']), a)
        assert got.dtype == np.float32 and np.array_equal(got, golden[f'bboxes_{a}']), a
    assert D.rotate_bboxes(np.zeros((0, 4), np.float32), (64, 64, 3), 90).shape == (0, 4)


def test_rotate_offsets_within_one_ulp_of_the_reference(golden):
    o = golden['offsets']
    assert o.shape[0] >= 16 and (o == 0).all(1).any() and np.hypot(o[:, 0], o[:, 1]).max() >= 199
    for a in ANGLES:
        got = D.rotate_offsets(golden['offsets'], a)
        assert got.dtype == np.float32 and got.shape == o.shape
        print(f'angle {a}: max distance {_ulps(got, golden[f"offsets_{a}"]).max()} ulp')
        assert _ulps(got, golden[f'offsets_{a}']).max() <= 1, a
    # not a sign swap: the polar round trip leaves cos(pi/2) * length in the other component
    assert D.rotate_offsets(np.array([[0, -100]], np.float32), 270)[0, 1] != 0


def _rect_sample(size=64, box=(10, 20, 30, 44), offset=(7, -5)):
    x1, y1, x2, y2 = box
    m = np.zeros((1, size, size), np.uint8)
    m[0, y1:y2, x1:x2] = 1
    img = np.random.RandomState(0).randint(0, 255, (size, size, 3)).astype(np.uint8)
    return dict(img=img, gt_bboxes=np.array([box], np.float32), gt_labels=np.zeros(1, np.int64), gt_masks=m,
                gt_offsets=np.array([offset], np.float32))


def _translate(m, dx, dy):
    """Bitmap [H, W] moved by whole pixels (dx to the right, dy down), zeros shifted in."""
    out = np.zeros_like(m)
    h, w = m.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = m[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


@pytest.mark.parametrize('angle', ANGLES)
def test_bitmap_box_and_offset_turn_the_same_way(angle):
    """An axis-aligned instance with integer corners strictly inside a 64 x 64 tile: the rows and columns its rotated bitmap
    occupies are its rotated box, the image turns with the bitmap, and translating by the offset commutes with the rotation."""
    s = _rect_sample()
    r = D.rotate_sample(s, angle)
    assert r['rotate'] is True and r['rotate_angle'] == angle
    m = r['gt_masks'][0]
    cols, rows = np.where(m.any(0))[0], np.where(m.any(1))[0]
    assert np.array_equal(r['gt_bboxes'][0], np.array([cols[0], rows[0], cols[-1] + 1, rows[-1] + 1], np.float32))
    assert m.sum() == s['gt_masks'].sum() and np.array_equal(r['img'], np.rot90(s['img'], k=-angle // 90))
    # the image and the bitmap are permuted alike: mark the instance in the image and find it under the rotated bitmap
    marked = dict(s, img=s['img'] * (1 - s['gt_masks'][0])[..., None])
    rm = D.rotate_sample(marked, angle)
    assert (rm['img'][rm['gt_masks'][0] == 1] == 0).all() and np.array_equal(rm['img'] == 0, np.rot90(marked['img'] == 0, k=-angle // 90))
    ox, oy = (int(v) for v in s['gt_offsets'][0])
    moved = D.rotate_sample(dict(s, gt_masks=_translate(s['gt_masks'][0], ox, oy)[None]), angle)['gt_masks'][0]
    rox, roy = (int(v) for v in np.round(r['gt_offsets'][0]))
    assert (rox, roy) != (ox, oy) or angle == 0
    assert np.array_equal(moved, _translate(m, rox, roy))


def test_four_quarter_turns_give_the_sample_back():
    s = _rect_sample()
    r = s
    for _ in range(4):
        r = D.rotate_sample(r, 90)
    assert np.array_equal(r['img'], s['img']) and np.array_equal(r['gt_masks'], s['gt_masks'])
    assert np.array_equal(r['gt_bboxes'], s['gt_bboxes'])
    print('offsets after four quarter turns:', r['gt_offsets'], _ulps(r['gt_offsets'], s['gt_offsets']))
    assert _ulps(r['gt_offsets'], s['gt_offsets']).max() <= 4
    assert D.d4_compose((90, 90, 90, 90)) == 0 and D.d4_compose((90, 90)) == D.d4_compose((180,)) == D.d4_compose(('horizontal', 'vertical'))


def test_flip_and_rotation_compose_in_order():
    """RandomFlip then RandomRotate is not RandomRotate then RandomFlip: host arrays and the deferred record (composed to one
    element of the square's symmetry group) both follow the numpy composition, in either order."""
    s = _rect_sample()
    poly = {k: v for k, v in s.items() if k != 'gt_masks'}
    poly['gt_polygons'] = [[[10, 20, 30, 20, 30, 44, 10, 44]]]
    fr = D.rotate_sample(D.flip_sample(s, 'horizontal'), 90)
    rf = D.flip_sample(D.rotate_sample(s, 90), 'horizontal')
    want_fr = lambda a, ax=(0, 1): np.rot90(np.flip(a, ax[1]), k=-1, axes=ax)
    want_rf = lambda a, ax=(0, 1): np.flip(np.rot90(a, k=-1, axes=ax), ax[1])
    assert np.array_equal(fr['img'], want_fr(s['img'])) and np.array_equal(rf['img'], want_rf(s['img']))
    assert np.array_equal(fr['gt_masks'], want_fr(s['gt_masks'], (1, 2))) and np.array_equal(rf['gt_masks'], want_rf(s['gt_masks'], (1, 2)))
    assert not np.array_equal(fr['img'], rf['img']) and not np.array_equal(fr['gt_masks'], rf['gt_masks'])
    assert not np.array_equal(fr['gt_bboxes'], rf['gt_bboxes']) and not np.array_equal(fr['gt_offsets'], rf['gt_offsets'])
    dfr = D.rotate_sample(D.flip_sample(poly, 'horizontal', defer_image=True), 90, defer_image=True)
    drf = D.flip_sample(D.rotate_sample(poly, 90, defer_image=True), 'horizontal', defer_image=True)
    assert dfr['img'] is s['img'] and dfr['img_flip'] == dfr['mask_flips'] == ('horizontal', 90)
    assert drf['img_flip'] == drf['mask_flips'] == (90, 'horizontal')
    e_fr, e_rf = D.d4_compose(dfr['img_flip']), D.d4_compose(drf['img_flip'])
    assert e_fr != e_rf
    assert np.array_equal(D.d4_apply(s['img'], e_fr), fr['img']) and np.array_equal(D.d4_apply(s['img'], e_rf), rf['img'])
    assert np.array_equal(D.d4_apply(s['gt_masks'], e_fr, axes=(1, 2)), fr['gt_masks'])
    assert np.array_equal(D.d4_apply(s['gt_masks'], e_rf, axes=(1, 2)), rf['gt_masks'])
    for k in ('gt_bboxes', 'gt_offsets'):
        assert np.array_equal(dfr[k], fr[k]) and np.array_equal(drf[k], rf[k])
    # every record of flips and right angles is one of the eight elements, and the eight are distinct
    a = np.arange(12).reshape(3, 4)[:3, :3]
    assert len({D.d4_apply(a, e).tobytes() for e in range(8)}) == 8
    for ops in [(90,), (180,), (270,), ('vertical', 270), (270, 'vertical', 90, 'horizontal', 180)]:
        want = a
        for op in ops:
            want = np.rot90(want, k=-op // 90) if not isinstance(op, str) else np.flip(want, 1 if op == 'horizontal' else 0)
        assert np.array_equal(D.d4_apply(a, D.d4_compose(ops)), want), ops
    # host tensors: a deferred rotation through to_device_batch equals the host-rotated sample through it
    hm = lambda smp: dict(smp, gt_masks=np.zeros((1, 64, 64), np.uint8))
    b_def = D.to_device_batch([hm({k: v for k, v in dfr.items() if k != 'gt_polygons'})], device='cpu')
    b_host = D.to_device_batch([hm(fr)], device='cpu')
    assert torch.equal(b_def['img'], b_host['img'])
    assert b_def['img_metas'][0]['rotate'] is True and b_def['img_metas'][0]['rotate_angle'] == 90 and b_def['img_metas'][0]['flip']


def _write_dataset(tmp_path, n_tiles=7, size=64):
    from PIL import Image
    from bonai_amd.synth import synth_bonai_anns
    rng = np.random.RandomState(1)
    images, annotations, aid = [], [], 0
    for i in range(n_tiles):
        name = f't{i}.png'
        Image.fromarray(rng.randint(0, 255, (size, size, 3)).astype(np.uint8)).save(tmp_path / name, compress_level=1)
        images.append(dict(id=i + 1, file_name=name, width=size, height=size))
        for a in (synth_bonai_anns(seed=i, size=size) if i != 2 else []):           # tile 2: no annotation -> replaced
            aid += 1
            annotations.append(dict(a, id=aid, image_id=i + 1))
    f = tmp_path / 'ann.json'
    json.dump(dict(images=images, annotations=annotations, categories=[dict(id=1, name='building')]), open(f, 'w'))
    return str(f)


def test_random_stream_is_unchanged_without_rotation_and_shared_by_the_loaders(tmp_path):
    from bonai_amd.dataset import BonaiDataset
    f = _write_dataset(tmp_path)
    raster = lambda polys, h, w: np.zeros((h, w), np.uint8)       # (bitmaps are not what this test is about)
    old = dict(filter_empty_gt=False, flip_ratio=0.5, flip_direction=['horizontal', 'vertical'], seed=3, img_scale=(64, 64),
               host_rasteriser=raster)
    order = [0, 2, 5, 2, 6, 1, 3, 4] * 3
    before = BonaiDataset(f, str(tmp_path), **old)                 # constructed the way callers do today
    want = [before.resolve(i) for i in order]
    assert len({d for _, d in want}) == len(want)                  # (real draws, not a constant)
    for kw in (dict(rotate_ratio=None), dict(rotate_ratio=0), dict(rotate_ratio=None, rotate_choice=(90,), rotate_first=True)):
        ds = BonaiDataset(f, str(tmp_path), **old, **kw)
        assert ds.flip_direction == before.flip_direction
        assert [ds.resolve(i) for i in order] == want
        ds = BonaiDataset(f, str(tmp_path), **old, **kw)
        assert [ds.resolve_all(i) for i in order] == [w + (None,) for w in want]
    a = BonaiDataset(f, str(tmp_path), **old)
    b = BonaiDataset(f, str(tmp_path), **old, rotate_ratio=None)
    for x, y in zip(a.batches(0, 2, device='cpu', seed=5), b.batches(0, 2, device='cpu', seed=5)):
        assert torch.equal(x['img'], y['img']) and [m['flip'] for m in x['img_metas']] == [m['flip'] for m in y['img_metas']]
        assert all(m['rotate'] is False and m['rotate_angle'] == 0 for m in y['img_metas'])
    # with rotation: the flip draw, then one draw against rotate_ratio, then a choice draw only for a rotated sample
    ds = BonaiDataset(f, str(tmp_path), **old, rotate_ratio=0.5)
    rng = np.random.RandomState(3)
    rng.choice(['horizontal', 'vertical'])
    for i in (0, 1, 3, 4, 5, 6) * 3:
        flip = float(rng.rand())
        angle = int(rng.choice((0, 90, 180, 270))) if rng.rand() < 0.5 else None
        assert ds.resolve_all(i) == (i, flip, angle)
    # the synchronous and the prefetching loader agree on every decision and on every value
    mk = lambda **kw: BonaiDataset(f, str(tmp_path), **old, rotate_ratio=0.5, **kw)
    for first in (False, True):
        a, b = mk(rotate_first=first), mk(rotate_first=first)
        seen = set()
        for epoch in range(2):
            sync = list(a.batches(epoch, 2, device='cpu', seed=5))
            pre = list(b.batches(epoch, 2, device='cpu', seed=5, prefetch=2, workers=3, processes=bool(epoch)))
            assert len(sync) == len(pre) == 4
            for x, y in zip(sync, pre):
                for key in ('filename', 'flip', 'flip_direction', 'rotate', 'rotate_angle'):
                    assert [m[key] for m in x['img_metas']] == [m[key] for m in y['img_metas']], key
                assert torch.equal(x['img'], y['img'])
                for k in ('gt_bboxes', 'gt_labels', 'gt_offsets'):
                    assert all(torch.equal(p, q) for p, q in zip(x[k], y[k]))
                seen |= {(m['flip'], m['rotate'], m['rotate_angle']) for m in x['img_metas']}
        b.close()
        assert {s[:2] for s in seen} == {(False, False), (False, True), (True, False), (True, True)}
        assert all(angle == 0 for _, rot, angle in seen if not rot) and len({angle for _, rot, angle in seen if rot}) >= 3


def test_unsupported_rotations_say_why(tmp_path):
    from bonai_amd.dataset import BonaiDataset
    f = _write_dataset(tmp_path, n_tiles=1)
    for choice in ((0, 45), 'any', [90, 359]):
        with pytest.raises(NotImplementedError, match='auto_bound=False'):
            BonaiDataset(f, str(tmp_path), img_scale=(64, 64), rotate_ratio=0.5, rotate_choice=choice)
    with pytest.raises(NotImplementedError, match='square'):
        BonaiDataset(f, str(tmp_path), img_scale=(96, 64), rotate_ratio=0.5)
    s = _rect_sample()
    wide = dict(s, img=np.zeros((64, 96, 3), np.uint8), gt_masks=np.zeros((1, 64, 96), np.uint8))       # a 96 x 64 tile
    for angle in (90, 270):
        with pytest.raises(NotImplementedError, match='square'):
            D.rotate_sample(wide, angle)
        with pytest.raises(NotImplementedError, match='square'):
            D.rotate_bboxes(s['gt_bboxes'], (64, 96, 3), angle)
    half = D.rotate_sample(wide, 180)                              # a half turn needs no square
    assert half['img'].shape == (64, 96, 3) and np.array_equal(half['gt_bboxes'], np.array([[96 - 30, 64 - 44, 96 - 10, 64 - 20]], np.float32))
    for angle in (45, -90, 360, 90.5):
        with pytest.raises(NotImplementedError):
            D.rotate_sample(s, angle)
    with pytest.raises(KeyError):
        D.rotate_sample({k: v for k, v in s.items() if k != 'gt_masks'}, 90)


def test_train_tool_reads_random_rotate_from_the_pipeline():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import train as train_tool
    finally:
        sys.path.pop(0)
    from bonai_amd.config import Config
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_rotate_2x_bonai.py'))
    head = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    assert cfg.model == head.model and cfg.optimizer == head.optimizer and cfg.data.samples_per_gpu == head.data.samples_per_gpu
    kw = train_tool.augment_kwargs(cfg.data.train.pipeline)
    assert kw == dict(flip_ratio=0.5, flip_direction=['horizontal', 'vertical'], rotate_ratio=0.5, rotate_choice=(0, 90, 180, 270),
                      rotate_first=False)
    assert train_tool.augment_kwargs([]) == dict(flip_ratio=0.0, flip_direction='horizontal')       # as before: nothing about rotation
    assert train_tool.augment_kwargs([dict(type='RandomFlip', flip_ratio=0.5)]) == dict(flip_ratio=0.5, flip_direction='horizontal')
    swapped = [dict(type='RandomRotate', rotate_ratio=0.25, choice=[90, 270]), dict(type='RandomFlip', flip_ratio=0.5, direction='vertical')]
    cfg.merge_from_dict(dict([train_tool.parse_option(f'data.train.pipeline={swapped!r}')]))
    kw = train_tool.augment_kwargs(cfg.data.train.pipeline)
    assert kw == dict(flip_ratio=0.5, flip_direction='vertical', rotate_ratio=0.25, rotate_choice=[90, 270], rotate_first=True)
