"""CPU: Resize and Pad on the host side.  Pins tests/resize_restatement.py (the statement the GPU tests hold the kernels to) to
answers worked out by hand and to the geometry of torch's bilinear interpolation, kernels.resize_tables to the restatement, and the
sample-level algebra of bonai_amd/data.py (mmcv's imrescale size rule, Resize's three scale draws, boxes, offsets) to values
computed by hand from the lines it cites.  Nothing here has been run against OpenCV or mmcv."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_restatement as RR  # noqa: E402

from bonai_amd import data as D  # noqa: E402
from bonai_amd import kernels as K  # noqa: E402


def test_equal_sizes_give_the_source_back():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (7, 9, 3)).astype(np.uint8)
    img[0, 0], img[0, 1] = 0, 255
    assert np.array_equal(RR.resize_linear(img, 7, 9), img)
    assert RR.linear_taps(9, 9) == [(i, 2048, 0) if i < 8 else (8, 2048, 0) for i in range(9)]
    m = rng.randint(0, 2, (2, 7, 9)).astype(np.uint8)
    assert np.array_equal(RR.resize_nearest(m, 7, 9), m)


def test_two_pixels_to_four():
    # dx = 0: fx = 0.5 * 0.5 - 0.5 = -0.25 -> sx = -1 -> clamped (0, fx = 0); dx = 1: 0.25; dx = 2: 0.75; dx = 3: 1.25 -> sx = 1 = Ws - 1
    assert RR.linear_taps(2, 4) == [(0, 2048, 0), (0, 1536, 512), (0, 512, 1536), (1, 2048, 0)]
    row = np.array([[[0], [200]]], np.uint8)                       # 1 x 2 x 1
    # rows: Hs = Hd = 1 -> b = (2048, 0).  S = 200 * 512 = 102400 -> >> 4 = 6400 -> * 2048 >> 16 = 200 -> (200 + 2) >> 2 = 50
    assert RR.resize_linear(row, 1, 4)[0, :, 0].tolist() == [0, 50, 150, 200]


def test_exact_half_is_the_mean_of_four():
    img = np.arange(16, dtype=np.uint8).reshape(4, 4, 1)
    # (0 + 1 + 4 + 5 + 2) >> 2 = 3, (2 + 3 + 6 + 7 + 2) >> 2 = 5, (8 + 9 + 12 + 13 + 2) >> 2 = 11, (10 + 11 + 14 + 15 + 2) >> 2 = 13
    assert RR.resize_linear(img, 2, 2)[:, :, 0].tolist() == [[3, 5], [11, 13]]
    img = np.array([[1, 2], [2, 2]], np.uint8).reshape(2, 2, 1)     # (7 + 2) >> 2 = 2: rounds half up
    assert RR.resize_linear(img, 1, 1)[0, 0, 0] == 2
    # only when BOTH sides halve: 4 x 4 -> 2 x 4 goes through the taps
    wide = RR.resize_linear(np.arange(16, dtype=np.uint8).reshape(4, 4, 1), 2, 4)[:, :, 0]
    # row 0: fy = 0.5 * 2 - 0.5 = 0.5 -> rows 0, 1 with (1024, 1024): columns are identities -> (v0 + v1) / 2 = 2, 3, 4, 5
    assert wide.tolist() == [[2, 3, 4, 5], [10, 11, 12, 13]]


def test_one_pixel_wide_source():
    assert RR.linear_taps(1, 5) == [(0, 2048, 0)] * 5
    col = np.array([[[10]], [[50]], [[90]]], np.uint8)              # 3 x 1 x 1
    assert np.array_equal(RR.resize_linear(col, 3, 4), np.repeat(col, 4, axis=1))
    assert RR.nearest_index(1, 4) == [0, 0, 0, 0]


def test_nearest_indices():
    # 5 -> 3: 1 / (3 / 5) = 1.666..: 0, 1.67, 3.33;   3 -> 7: 1 / (7 / 3) = 0.428..: 0, .43, .86, 1.29, 1.71, 2.14, 2.57
    assert RR.nearest_index(5, 3) == [0, 1, 3]
    assert RR.nearest_index(3, 7) == [0, 0, 0, 1, 1, 2, 2]
    m = np.arange(5, dtype=np.uint8).reshape(1, 1, 5)
    assert RR.resize_nearest(m, 1, 3)[0, 0].tolist() == [0, 1, 3]


@pytest.mark.parametrize('src, dst', [((37, 53), (64, 48)), ((53, 37), (20, 90)), ((64, 64), (200, 200))])
def test_geometry_against_torch_bilinear(src, dst):
    """Within 1 grey level of the rounded float result: the integer rule is within 0.125 + 0.0625 (coefficients) + 0.5 (two
    truncations) + 0.5 (final rounding) of the real value.  More than that is wrong geometry."""
    rng = np.random.RandomState(src[0] * 1000 + dst[0])
    img = rng.randint(0, 256, src + (3,)).astype(np.uint8)
    got = RR.resize_linear(img, *dst).astype(np.int64)
    ref = torch.nn.functional.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None].double(), size=dst, mode='bilinear',
                                          align_corners=False)[0].permute(1, 2, 0).numpy()
    diff = np.abs(got - np.rint(ref))
    print('max |integer rule - rint(float bilinear)| =', diff.max())
    assert diff.max() <= 1


@pytest.mark.parametrize('src, dst', [((37, 53), (64, 48)), ((96, 96), (12, 12)), ((64, 64), (33, 33)), ((1, 9), (4, 4)), ((9, 1), (5, 3)),
                                      ((1024, 1024), (768, 768)), ((1000, 600), (1333, 800))])
def test_table_builder_equals_the_restatement(src, dst):
    t = K.resize_tables(src[0], src[1], dst[0], dst[1])
    for ofs, coef, idx, S, Dn in (('xofs', 'xcoef', 'xidx', src[1], dst[1]), ('yofs', 'ycoef', 'yidx', src[0], dst[0])):
        taps = RR.linear_taps(S, Dn)
        assert t[ofs].dtype == np.int32 and t[coef].dtype == np.int16 and t[idx].dtype == np.int32 and t[coef].shape == (Dn, 2)
        assert t[ofs].tolist() == [a[0] for a in taps]
        assert t[coef].tolist() == [[a[1], a[2]] for a in taps]
        assert t[idx].tolist() == RR.nearest_index(S, Dn)


def test_rescale_size_by_hand():
    # 96 x 96 -> (128, 128): s = 128 / 96; int(96 * s + 0.5) = int(128.5) = 128
    assert D.rescale_size((96, 96), (128, 128)) == (128, 128)
    # w = 1000, h = 600, (1333, 800): s = min(1333 / 1000, 800 / 600) = 1.333 -> int(1333.5) = 1333, int(799.8 + 0.5) = 800
    assert D.rescale_size((1000, 600), (1333, 800)) == (1333, 800)
    assert D.rescale_size((1000, 600), (800, 1333)) == (1333, 800)               # the scale's own order does not matter
    # w = 100, h = 300, (200, 100): s = min(200 / 300, 100 / 100) = 2 / 3 -> int(66.67 + 0.5) = 67, int(200.5) = 200
    assert D.rescale_size((100, 300), (200, 100)) == (67, 200)
    g = D.resize_geometry((300, 100), (200, 100), keep_ratio=True, pad_divisor=32)
    assert g['size'] == (200, 67) and g['pad'] == (224, 96) and g['w_scale'] == 67 / 100 and g['h_scale'] == 200 / 300
    g = D.resize_geometry((300, 100), (50, 90), keep_ratio=False, pad_divisor=None)       # imresize: (w, h) as given
    assert g['size'] == (90, 50) and g['pad'] == (90, 50) and g['w_scale'] == 0.5 and g['h_scale'] == 0.3


def test_scale_draws_make_the_cited_numpy_calls():
    scales = [(1333, 640), (1333, 800), (1000, 700)]
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    for _ in range(4):                                               # transforms.py:100-101
        assert D.random_select(scales, a) == scales[b.randint(len(scales))]
    for _ in range(4):                                               # :120-128: long edge first, then short edge
        got = D.random_sample([(1333, 640), (1000, 800)], a)
        assert got == (b.randint(1000, 1334), b.randint(640, 801))
    for _ in range(4):                                               # :154-155
        got = D.random_sample_ratio((1000, 600), (0.5, 1.5), a)
        ratio = b.random_sample() * (1.5 - 0.5) + 0.5
        assert got == (int(1000 * ratio), int(600 * ratio))
    # _random_scale's order of cases (:176-186); a single scale draws nothing
    assert D.random_scale([(128, 128)], 'range', None, a) == (128, 128)
    assert a.get_state()[2] == b.get_state()[2] and np.array_equal(a.get_state()[1], b.get_state()[1])
    assert D.random_scale([(128, 128)], 'range', (1.0, 1.0), a) == (128, 128) and b.random_sample() >= 0
    assert D.random_scale(scales, 'value', None, a) == scales[b.randint(3)]
    assert D.random_scale(scales[:2], 'range', None, a) == (b.randint(1333, 1334), b.randint(640, 801))
    with pytest.raises(ValueError):
        D.random_sample(scales, a)


def _sample(h=60, w=100):
    return dict(img=np.zeros((h, w, 3), np.uint8), gt_bboxes=np.array([[10, 20, 50, 40], [95, 55, 104, 62]], np.float32),
                gt_labels=np.zeros(2, np.int64), gt_polygons=[[[10, 20, 50, 20, 50, 40]], [[95, 55, 104, 55, 104, 62]]],
                gt_offsets=np.array([[2, -4], [0.5, 8]], np.float32))


def test_resize_sample_by_hand():
    # 100 x 60 under (150, 90), keep_ratio: s = min(150 / 100, 90 / 60) = 1.5 -> 150 x 90, padded to 160 x 96
    out = D.resize_sample(_sample(), (150, 90), keep_ratio=True, pad_divisor=32)
    assert out['resize']['size'] == (90, 150) and out['resize']['pad'] == (96, 160) and out['img_shape'] == (90, 150, 3)
    assert out['scale_factor'].dtype == np.float32 and out['scale_factor'].tolist() == [1.5, 1.5, 1.5, 1.5]
    # second box: (142.5, 82.5, 156, 93) clipped to x <= 150, y <= 90 (_resize_bboxes, transforms.py:226-228)
    assert out['gt_bboxes'].dtype == np.float32 and out['gt_bboxes'].tolist() == [[15, 30, 75, 60], [142.5, 82.5, 150, 90]]
    # the deviation: offsets are scaled (the reference leaves them)
    assert out['gt_offsets'].dtype == np.float32 and out['gt_offsets'].tolist() == [[3, -6], [0.75, 12]]
    assert out['img'].shape == (60, 100, 3)                          # pixels stay at the source size
    # keep_ratio=False, (50, 90): w_scale = 0.5, h_scale = 1.5, each on its own axis
    out = D.resize_sample(_sample(), (50, 90), keep_ratio=False, pad_divisor=32)
    assert out['scale_factor'].tolist() == [0.5, 1.5, 0.5, 1.5] and out['resize']['pad'] == (96, 64)
    assert out['gt_bboxes'].tolist() == [[5, 30, 25, 60], [47.5, 82.5, 50, 90]]
    assert out['gt_offsets'].tolist() == [[1, -6], [0.25, 12]]
    # the float32 factor, not the float64 quotient, multiplies the boxes: 67 / 100 in float32
    out = D.resize_sample(_sample(300, 100), (200, 100))
    assert out['gt_bboxes'][0, 0] == np.float32(10) * np.float32(67 / 100)


def test_flips_of_a_resized_sample_use_its_own_frame():
    out = D.resize_sample(_sample(), (150, 90))
    fl = D.flip_sample(out, 'horizontal', defer_image=True)
    assert fl['gt_bboxes'][0].tolist() == [150 - 75, 30, 150 - 15, 60] and fl['img_flip'] == ('horizontal',)
    assert fl['mask_flips'] == ('horizontal',) and fl['gt_offsets'][0].tolist() == [-3, -6]
    with pytest.raises(ValueError, match='deferred'):
        D.flip_sample(out, 'horizontal')
    with pytest.raises(ValueError, match='comes first'):
        D.resize_sample(D.flip_sample(_sample(), 'vertical', defer_image=True), (150, 90))


def _ann_file(tmp_path, sizes=(96, 96, 96), name='ann.json'):
    from bonai_amd.synth import synth_bonai_anns
    images, annotations, aid = [], [], 0
    for i, size in enumerate(sizes):
        images.append(dict(id=10 + i, file_name=f'tile_{i}.png', width=size, height=size))
        for a in synth_bonai_anns(seed=i, size=size):
            aid += 1
            annotations.append(dict(a, id=aid, image_id=10 + i))
    f = tmp_path / name
    json.dump(dict(images=images, annotations=annotations, categories=[dict(id=1, name='building')]), open(f, 'w'))
    return str(f)


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


def test_without_resize_the_random_stream_is_the_old_one(tmp_path):
    """resize=None draws what the loader drew before Resize existed: one ``choice`` for the direction list when the dataset is
    built, one uniform draw per sample.  A fixed scale adds nothing; a scale list adds ONE randint per batch, before the flips."""
    from bonai_amd.dataset import BonaiDataset
    f = _ann_file(tmp_path)
    want = np.random.RandomState(3)
    want.choice(['horizontal', 'vertical'])
    ds = BonaiDataset(f, str(tmp_path), seed=3, img_scale=(96, 96))
    assert ds.resize is None and ds.draw_scale() is None and _same_state(ds.rng, want)
    draws = [ds.resolve_all(i) for i in range(3)]
    assert draws == [(i, float(want.rand()), None) for i in range(3)] and _same_state(ds.rng, want)
    fixed = BonaiDataset(f, str(tmp_path), seed=3, resize=dict(img_scale=(128, 128), keep_ratio=True))
    assert fixed.draw_scale() == (128, 128) and [fixed.resolve_all(i) for i in range(3)] == draws
    multi = BonaiDataset(f, str(tmp_path), seed=3, resize=dict(img_scale=[(64, 64), (128, 128)], multiscale_mode='value'))
    want = np.random.RandomState(3)
    want.choice(['horizontal', 'vertical'])
    assert multi.multi_scale and not fixed.multi_scale
    assert multi.draw_scale() == [(64, 64), (128, 128)][want.randint(2)]
    assert multi.resolve_all(0) == (0, float(want.rand()), None) and _same_state(multi.rng, want)


def test_dataset_refusals_that_need_no_device(tmp_path):
    from bonai_amd.dataset import BonaiDataset
    f = _ann_file(tmp_path)
    rs = dict(img_scale=(128, 128))
    with pytest.raises(NotImplementedError, match='mixed source sizes'):
        BonaiDataset(_ann_file(tmp_path, (96, 96, 64), 'mixed.json'), str(tmp_path), resize=rs)
    with pytest.raises(NotImplementedError, match='pillow'):
        BonaiDataset(f, str(tmp_path), resize=dict(rs, backend='pillow'))
    with pytest.raises(NotImplementedError, match='bilinear'):
        BonaiDataset(f, str(tmp_path), resize=dict(rs, interpolation='bicubic'))
    with pytest.raises(NotImplementedError, match='test_views'):
        BonaiDataset(f, str(tmp_path), test_mode=True, resize=rs, test_views=[None, 'horizontal'], img_scale=(96, 96))
    with pytest.raises(NotImplementedError, match='multi-scale test views'):
        BonaiDataset(f, str(tmp_path), test_mode=True, resize=dict(img_scale=[(64, 64), (128, 128)], multiscale_mode='value'))
    with pytest.raises(NotImplementedError, match='pad_divisor=64'):
        BonaiDataset(f, str(tmp_path), resize=dict(img_scale=(96, 96)))                   # 96 = 3 * 32: an odd P5
    assert BonaiDataset(f, str(tmp_path), resize=dict(img_scale=(96, 96)), pad_divisor=64)._geometry((96, 96))['pad'] == (128, 128)
    with pytest.raises(NotImplementedError, match='square target'):
        BonaiDataset(f, str(tmp_path), resize=dict(rs, keep_ratio=False), rotate_ratio=0.5)
    with pytest.raises(NotImplementedError, match='ONE scale'):
        a, b = D.resize_sample(_sample(), (150, 90)), D.resize_sample(_sample(), (100, 60))
        D.to_device_batch([a, b], device='cpu')
