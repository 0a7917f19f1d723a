"""CPU: test-time augmentation -- config / CLI parsing to view lists, the view algebra, the torch restatement of the merges against
the reference's own outputs (tests/golden/tta_ops.npz, written by tools/make_tta_goldens.py), and the detector's dispatch."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_restatement as T  # noqa: E402

from bonai_amd import tta  # noqa: E402
from bonai_amd.data import d4_apply, d4_compose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _pipeline(**aug):
    return [dict(type='LoadImageFromFile'), dict(type='MultiScaleFlipAug', transforms=[], **aug)]


def _write_dataset(tmp_path, size=32):
    from PIL import Image
    rng = np.random.RandomState(1)
    images = []
    for i in range(2):
        Image.fromarray(rng.randint(0, 255, (size, size, 3)).astype(np.uint8)).save(tmp_path / f't{i}.png', compress_level=1)
        images.append(dict(id=i + 1, file_name=f't{i}.png', width=size, height=size))
    f = tmp_path / 'ann.json'
    json.dump(dict(images=images, annotations=[], categories=[dict(id=1, name='building')]), open(f, 'w'))
    return str(f)


def test_config_and_cli_to_view_lists(tmp_path):
    from bonai_amd.dataset import BonaiDataset
    both = tta.views_from_pipeline(_pipeline(img_scale=(1024, 1024), flip=True, flip_direction=['horizontal', 'vertical']))
    assert both == [None, 'horizontal', 'vertical']                            # the reference's order: unflipped first
    assert tta.views_from_pipeline(_pipeline(img_scale=(1024, 1024), flip=True)) == [None, 'horizontal']
    assert tta.views_from_pipeline(_pipeline(img_scale=(1024, 1024), flip=True, flip_direction='vertical',
                                             rotate_angles=(270, 90))) == [None, 'vertical', 270, 90]
    assert tta.views_from_pipeline(_pipeline(img_scale=(1024, 1024), flip=False)) is None
    assert tta.views_from_pipeline([dict(type='LoadImageFromFile')]) is None
    assert tta.parse_tta_arg('h,v,r90,r180,r270') == [None, 'horizontal', 'vertical', 90, 180, 270]
    assert tta.parse_tta_arg('r180, h') == [None, 'horizontal', 180]
    assert [tta.view_element(v) for v in tta.parse_tta_arg('h,v,r90,r180,r270')] == [0, 2, 4, 3, 6, 5]
    with pytest.raises(ValueError):
        tta.parse_tta_arg('h,x')
    with pytest.raises(NotImplementedError, match='img_scale'):
        tta.views_from_pipeline(_pipeline(img_scale=[(1024, 1024), (512, 512)], flip=True))
    with pytest.raises(NotImplementedError, match='img_scale'):
        tta.views_from_pipeline(_pipeline(img_scale=(512, 512), flip=True))
    with pytest.raises(NotImplementedError, match='scale_factor'):
        tta.views_from_pipeline(_pipeline(scale_factor=[1.0, 2.0], flip=True))
    with pytest.raises(NotImplementedError, match='square'):
        tta.views_from_pipeline(_pipeline(img_scale=(96, 64), flip=False, rotate_angles=(90,)), tile=(64, 96))
    assert tta.views_from_pipeline(_pipeline(img_scale=(96, 64), flip=True, rotate_angles=(180,)), tile=(64, 96)) == [None, 'horizontal', 180]
    with pytest.raises(NotImplementedError):
        tta.make_views(rotate_angles=(45,))
    # flip=False: exactly today's test_batches output
    f = _write_dataset(tmp_path)
    plain = list(BonaiDataset(f, str(tmp_path), test_mode=True, img_scale=(32, 32)).test_batches(device='cpu'))
    same = list(BonaiDataset(f, str(tmp_path), test_mode=True, img_scale=(32, 32),
                             test_views=tta.views_from_pipeline(_pipeline(img_scale=(32, 32), flip=False), tile=(32, 32))
                             ).test_batches(device='cpu'))
    assert len(plain) == len(same) == 2
    for (i, a), (j, b) in zip(plain, same):
        assert i == j and len(b['img']) == 1 and torch.equal(a['img'][0], b['img'][0])
        assert a['img_metas'][0][0].keys() == b['img_metas'][0][0].keys() and tta.META_KEY not in b['img_metas'][0][0]
    with pytest.raises(NotImplementedError, match='square'):
        BonaiDataset(f, str(tmp_path), test_mode=True, img_scale=(64, 32), test_views=[None, 90])


def test_view_algebra():
    probe = np.arange(12).reshape(3, 4)
    sq = np.arange(9).reshape(3, 3)
    for e in range(8):
        inv = tta.d4_inverse(e)
        a = sq if e & 1 else probe
        assert np.array_equal(d4_apply(d4_apply(a, e), inv), a), e
    rng = np.random.RandomState(0)
    for (H, W) in ((64, 96), (64, 64)):
        x, y = rng.randint(-5, W, 50), rng.randint(-5, H, 50)
        b = np.stack([x, y, x + rng.randint(0, 40, 50), y + rng.randint(0, 40, 50)], 1).astype(np.float32)
        for e in range(8):
            if e & 1 and H != W:
                continue
            v = tta.map_boxes(b, e, (H, W))
            assert np.array_equal(tta.map_boxes(v, e, (H, W), back=True), b), e          # to the bit on integer-valued boxes
            tb = torch.from_numpy(b)
            assert np.array_equal(T.boxes_to_view(tb, e, H, W).numpy(), v)
            assert np.array_equal(T.boxes_from_view(torch.from_numpy(v), e, H, W).numpy(), b)
            # the box of a painted rectangle follows the image permutation
            img = np.zeros((H, W), np.uint8)
            bx = np.array([[3, 5, 20, 30]], np.float32)
            img[5:30, 3:20] = 1
            ys, xs = np.nonzero(d4_apply(img, e))
            assert [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] == tta.map_boxes(bx, e, (H, W))[0].tolist(), e
    # against the reference's own RandomRotate (tests/golden/random_rotate.npz): offset_rotate is a float64 polar round trip and
    # bbox_rotate a float64 matrix product cast to float32, the view maps are exact sign swaps / subtractions -- they agree to the
    # round trip's rounding: a few ulp of the vector's length (atol 4 * 2^-23 * 200 px) / of the 1024 px tile for the boxes
    g = np.load(os.path.join(GOLD, 'random_rotate.npz'))
    size = int(g['img_shape'][0])
    for angle in (90, 180, 270):
        e = d4_compose([angle])
        assert np.allclose(tta.map_offsets(g['offsets'], e), g[f'offsets_{angle}'], rtol=0, atol=1e-4), angle
        assert np.array_equal(tta.map_offsets(tta.map_offsets(g['offsets'], e), e, back=True), g['offsets'])
        assert np.allclose(tta.map_boxes(g['bboxes'], e, (size, size)), g[f'bboxes_{angle}'], rtol=0, atol=5e-4), angle
        o = torch.from_numpy(g['offsets'])
        assert np.array_equal(T.offsets_from_view(torch.from_numpy(tta.map_offsets(g['offsets'], e)), e).numpy(), o.numpy())


def test_restatement_equals_the_reference_fixture_bit_for_bit():
    g = np.load(os.path.join(GOLD, 'tta_ops.npz'))
    H, W = int(g['img_shape'][0]), int(g['img_shape'][1])
    elem = {None: 0, 'horizontal': tta.view_element('horizontal'), 'vertical': tta.view_element('vertical')}
    boxes = torch.from_numpy(g['boxes'])
    for d, e in elem.items():
        assert np.array_equal(T.boxes_to_view(boxes, e, H, W).numpy(), g[f'mapping_{d}']), d
        assert np.array_equal(T.boxes_from_view(boxes, e, H, W).numpy(), g[f'mapping_back_{d}']), d
        assert np.array_equal(tta.map_boxes(g['boxes'], e, (H, W)), g[f'mapping_{d}']), d
        rois = T.view_rois(boxes, [e], H, W)
        assert np.array_equal(rois[:, 1:].numpy(), g[f'mapping_{d}']) and (rois[:, 0] == 0).all()
    for V in (2, 3):
        elems = [0, elem['horizontal'], elem['vertical']][:V]
        mb, ms = T.merge_view_bboxes(list(torch.from_numpy(g[f'bboxes_in_{V}'])), list(torch.from_numpy(g[f'scores_in_{V}'])), elems, H, W)
        assert np.array_equal(mb.numpy(), g[f'bboxes_out_{V}']) and np.array_equal(ms.numpy(), g[f'scores_out_{V}']), V
        mm = T.merge_masks(torch.from_numpy(g[f'masks_in_{V}'])[:, :, 0], elems)
        assert np.array_equal(mm.numpy(), g[f'masks_out_{V}'][:, 0]), V
        props = torch.from_numpy(g[f'props_in_{V}'])
        counts = torch.full((V,), props.shape[1], dtype=torch.int64)
        got = T.merge_proposals(props, counts, elems, H, W, float(g['rpn_nms_thr']), int(g['rpn_max_num']))
        assert np.array_equal(got.numpy(), g[f'props_out_{V}']), V


class _Stub(torch.nn.Module):
    from bonai_amd.loft.detector import LOFT
    forward_test = LOFT.forward_test

    def __init__(self):
        super().__init__()
        self.calls = []

    def aug_test(self, imgs, img_metas, **kw):
        self.calls.append(('aug', len(imgs), kw))
        return 'aug'

    def simple_test(self, img, img_metas, **kw):
        self.calls.append(('simple', 1, kw))
        return 'simple'


def test_forward_test_dispatches_three_views_to_aug_test():
    m = _Stub()
    imgs = [torch.zeros(1, 3, 8, 8) for _ in range(3)]
    metas = [[tta.view_meta(dict(img_shape=(8, 8, 3), pad_shape=(8, 8, 3), ori_shape=(8, 8, 3)), op)] for op in (None, 'horizontal', 90)]
    assert m.forward_test(imgs, metas, rescale=True) == 'aug' and m.calls == [('aug', 3, dict(rescale=True))]
    assert m.forward_test(imgs[:1], metas[:1], rescale=True) == 'simple' and m.calls[-1][0] == 'simple'
    assert [tta.meta_element(x[0]) for x in metas] == [0, 2, 3]
    assert tta.meta_element(dict(flip=True, flip_direction='vertical')) == 4          # a hand-built meta without the key
    assert metas[2][0]['rotate'] and metas[2][0]['rotate_angle'] == 90 and not metas[2][0]['flip']
