"""GPU: Resize and Pad on the device (bonai_amd/csrc/resize.hip).  loft_image_resize_prep_d4 and loft_mask_resize_d4_u8 against
tests/resize_restatement.py, bit for bit (the float outputs come from integers through the Normalize statement the restatement
repeats in float32); the loader with ``resize`` against the restatement applied to the decoded tiles; inference on a resized tile
against the same model on the restatement-resized image fed as a native tile; and the refusals."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_restatement as RR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
INVALID_VALUE = 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _image_case(src, size, pad, elems, keeps, seed=0):
    from bonai_amd import kernels as K
    rng = np.random.RandomState(seed)
    imgs = rng.randint(0, 256, (len(elems),) + tuple(src) + (3,)).astype(np.uint8)
    imgs[:, 0, 0], imgs[:, -1, -1] = 0, 255
    got = K.image_resize_prep(torch.from_numpy(imgs).cuda(), size, pad, elems, keeps, MEAN, STD)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(elems), 3) + tuple(pad) and got.is_contiguous()
    got = got.cpu().numpy()
    for i, (e, k) in enumerate(zip(elems, keeps)):
        want = RR.image_prep(imgs[i], size, pad, e, k, MEAN, STD)
        assert np.array_equal(_bits(got[i]), _bits(want)), (src, size, pad, e, k, np.abs(got[i] - want).max())
    return imgs, got


IMAGE_CASES = {
    'keep_ratio_false_37x53_to_64x48': ((37, 53), (64, 48), (64, 64), [0, 6]),
    'exact_half_64_to_32': ((64, 64), (32, 32), (32, 32), [0, 3]),
    'just_off_the_half_64_to_33': ((64, 64), (33, 33), (64, 64), [0, 5]),
    'taps_skip_pixels_96_to_12': ((96, 96), (12, 12), (32, 32), [0, 7]),
    'source_1x9': ((1, 9), (5, 20), (32, 32), [0, 2]),
    'source_9x1': ((9, 1), (20, 5), (32, 32), [0, 4]),
    'upscale_over_several_tiles_50x70_to_130x100': ((50, 70), (130, 100), (160, 128), [0, 6]),
}


@pytest.mark.parametrize('name', sorted(IMAGE_CASES))
def test_image_kernel_equals_the_restatement(name):
    src, size, pad, elems = IMAGE_CASES[name]
    _image_case(src, size, pad, elems, [False, True], seed=len(name))


@pytest.mark.parametrize('src', [(64, 64), (72, 100)])
def test_identity_size_is_image_prep_d4(src):
    """At the source's own size the new kernel gives the restatement's output AND loft_image_prep_d4's for the same element, bit
    for bit: a0 = 2048, a1 = 0 gives the byte back, and both kernels call one Normalize statement."""
    from bonai_amd import kernels as K
    elems = list(range(8)) if src[0] == src[1] else [0, 2, 4, 6]
    keeps = [bool(e & 2) for e in elems]
    imgs, got = _image_case(src, src, src, elems, keeps, seed=src[1])
    old = K.image_prep_d4(torch.from_numpy(imgs).cuda(), elems, keeps, MEAN, STD)
    assert np.array_equal(_bits(old.cpu().numpy()), _bits(got))


def test_all_eight_elements_on_a_square_target():
    _image_case((50, 70), (72, 72), (96, 96), list(range(8)), [False] * 8, seed=8)


def test_pad_is_exactly_zero():
    _, got = _image_case((33, 41), (50, 70), (64, 96), [0, 2, 4, 6], [False, True, False, True], seed=5)
    pad = np.concatenate([got[:, :, 50:, :].reshape(-1), got[:, :, :, 70:].reshape(-1)])
    assert pad.size and (_bits(pad) == 0).all()              # +0.0f, not -0.0f, not (0 - mean) / std


def test_batch_of_three_with_different_elements_and_channel_orders():
    _image_case((40, 40), (56, 56), (64, 64), [1, 6, 0], [True, False, True], seed=3)


MASK_CASES = dict(IMAGE_CASES, identity_64=((64, 64), (64, 64), (64, 64), list(range(8))),
                  square_target_all_elements=((50, 70), (72, 72), (96, 96), list(range(8))),
                  padded_50x70_on_64x96=((33, 41), (50, 70), (64, 96), [0, 2, 4, 6]))


@pytest.mark.parametrize('name', sorted(MASK_CASES))
def test_mask_kernel_equals_the_restatement(name):
    from bonai_amd import kernels as K
    src, size, pad, elems = MASK_CASES[name]
    rng = np.random.RandomState(len(name))
    m = np.array([0, 1, 255], np.uint8)[rng.randint(0, 3, (3,) + tuple(src))]
    dev = torch.from_numpy(m).cuda()
    for e in elems:
        got = K.mask_resize_u8(dev, size, pad, e)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3,) + tuple(pad) and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), RR.mask_prep(m, size, pad, e)), (name, e)
    assert tuple(K.mask_resize_u8(dev[:0], size, pad, 0).shape) == (0,) + tuple(pad)


def test_argument_contract_is_checked_before_any_launch():
    """hipErrorInvalidValue from the entry points, nothing launched (the pointers are never read: NULL)."""
    from bonai_amd import kernels as K, lib as L
    lib = L.load()
    tail = (*MEAN, *STD, None, None)
    assert lib.loft_image_resize_prep_d4(None, None, 1, 8, 8, 16, 16, None, None, None, None, 8, 16, 0, *tail) == INVALID_VALUE   # Hd > Hp
    assert lib.loft_image_resize_prep_d4(None, None, 1, 8, 8, 16, 12, None, None, None, None, 16, 16, 1, *tail) == INVALID_VALUE  # transpose
    assert lib.loft_image_resize_prep_d4(None, None, 1, 0, 8, 16, 16, None, None, None, None, 16, 16, 0, *tail) == INVALID_VALUE
    assert lib.loft_image_resize_prep_d4(None, None, 0, 8, 8, 16, 16, None, None, None, None, 16, 16, 0, *tail) == 0
    assert lib.loft_mask_resize_d4_u8(None, 1, 8, 8, 16, 16, None, None, 16, 18, 0, None, None) == INVALID_VALUE                  # Wp % 4
    assert lib.loft_mask_resize_d4_u8(None, 1, 8, 8, 16, 12, None, None, 16, 16, 1, None, None) == INVALID_VALUE
    assert lib.loft_mask_resize_d4_u8(None, 1, 8, 8, 16, 16, None, None, 16, 16, 8, None, None) == INVALID_VALUE
    assert lib.loft_mask_resize_d4_u8(None, 0, 8, 8, 16, 16, None, None, 16, 16, 3, None, None) == 0
    with pytest.raises(L.LoftHipError):
        K.image_resize_prep(torch.zeros(1, 8, 8, 3, dtype=torch.uint8).cuda(), (16, 12), (16, 16), [1], [False], MEAN, STD)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the loader
SRC = 96


def _dataset_files(tmp_path, sizes=(SRC, SRC, SRC), name='ann.json'):
    from PIL import Image
    from bonai_amd.synth import synth_bonai_anns
    rng = np.random.RandomState(0)
    images, annotations, aid = [], [], 0
    for i, size in enumerate(sizes):
        fn = f'tile_{i}_{size}.png'
        Image.fromarray(rng.randint(0, 255, (size, size, 3)).astype(np.uint8)).save(tmp_path / fn, compress_level=1)
        images.append(dict(id=10 + i, file_name=fn, width=size, height=size))
        for a in synth_bonai_anns(seed=i, size=size):
            aid += 1
            annotations.append(dict(a, id=aid, image_id=10 + i))
    f = tmp_path / name
    json.dump(dict(images=images, annotations=annotations, categories=[dict(id=1, name='building')]), open(f, 'w'))
    return str(f)


def _rgb(tmp_path, info):
    from PIL import Image
    return np.asarray(Image.open(tmp_path / info['filename']).convert('RGB'))


def test_training_loader_equals_the_restatement(tmp_path):
    """Three 96 x 96 tiles under Resize((128, 128), keep_ratio) and a horizontal flip, prefetching on and off: image, boxes, offsets
    and bitmaps are the restatement's on the decoded tiles; a Trainer step on the batch gives finite losses."""
    from bonai_amd import kernels as K
    from bonai_amd.config import Config
    from bonai_amd.dataset import BonaiDataset
    from bonai_amd.engine import Trainer
    from bonai_amd.loft import build_detector
    f = _dataset_files(tmp_path)
    ds = BonaiDataset(f, str(tmp_path), flip_ratio=1.0, flip_direction='horizontal', seed=1,
                      resize=dict(img_scale=(128, 128), keep_ratio=True))
    factor = np.float32(128 / 96)
    want = []
    for i in range(3):
        ann = ds.get_ann_info(i)
        boxes = np.clip(ann['bboxes'] * factor, 0, 128)                                 # _resize_bboxes, then bbox_flip
        boxes = np.stack([128 - boxes[:, 2], boxes[:, 1], 128 - boxes[:, 0], boxes[:, 3]], 1).astype(np.float32)
        offsets = (ann['offsets'] * factor * np.array([-1, 1], np.float32)).astype(np.float32)
        bitmaps = RR.mask_prep(K.poly2mask(ann['masks'], SRC, SRC).cpu().numpy(), (128, 128), (128, 128), RR.FX)
        want.append((RR.image_prep(_rgb(tmp_path, ds.data_infos[i]), (128, 128), (128, 128), RR.FX, True, MEAN, STD), boxes, offsets, bitmaps))
    batch = None
    for prefetch in (0, 2):
        it = ds.batches(0, 3, shuffle=False, prefetch=prefetch, workers=2, processes=False)
        batch = next(it)
        it.close()
        torch.cuda.synchronize()
        assert tuple(batch['img'].shape) == (3, 3, 128, 128)
        for i, (img, boxes, offsets, bitmaps) in enumerate(want):
            assert np.array_equal(_bits(batch['img'][i].cpu().numpy()), _bits(img)), (prefetch, i)
            assert np.array_equal(batch['gt_bboxes'][i].cpu().numpy(), boxes), (prefetch, i)
            assert np.array_equal(batch['gt_offsets'][i].cpu().numpy(), offsets), (prefetch, i)
            assert np.array_equal(batch['gt_masks'][i].cpu().numpy(), bitmaps) and bitmaps.any(), (prefetch, i)
            m = batch['img_metas'][i]
            assert m['ori_shape'] == (SRC, SRC, 3) and m['img_shape'] == (128, 128, 3) and m['pad_shape'] == (128, 128, 3)
            assert m['scale_factor'].dtype == np.float32 and (m['scale_factor'] == factor).all() and m['keep_ratio'] and m['flip']
    ds.close()
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    torch.manual_seed(0)
    model = build_detector(dict(cfg.model, pretrained=None), train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().train()
    lv = dict(Trainer(model, lr=1e-3).train_step(batch)['log_vars'].items())
    assert all(np.isfinite(v) for v in lv.values()), lv


def test_multiscale_value_draws_one_size_per_batch(tmp_path):
    from bonai_amd.dataset import BonaiDataset
    f = _dataset_files(tmp_path)
    ds = BonaiDataset(f, str(tmp_path), flip_ratio=0.5, seed=2, resize=dict(img_scale=[(64, 64), (128, 128)], multiscale_mode='value'))
    seen = set()
    for epoch in range(4):
        for batch in ds.batches(epoch, 2, shuffle=False):
            side = batch['img'].shape[-1]
            assert tuple(batch['img'].shape) == (2, 3, side, side)
            assert all(m['img_shape'] == (side, side, 3) for m in batch['img_metas'])
            assert all(tuple(m.shape[1:]) == (side, side) for m in batch['gt_masks'])
            seen.add(side)
    assert seen == {64, 128}


# ---------------------------------------------------------------------------------------------------------------- inference
@pytest.fixture(scope='module')
def model():
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    cfg.test_cfg.rcnn.max_per_img = 40
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    return m.cuda().eval()


def test_inference_on_a_resized_tile_equals_the_native_run(tmp_path, model):
    """A 96 x 96 tile through test_batches + forward_test(rescale=True) against the same model on the restatement-resized 128 x 128
    image fed as a native tile: boxes are the native ones divided by the factor in fp32, scores equal, masks pasted on 96 x 96 are
    mask_paste of the native logits (of the RoIs the result stage forms) at the divided boxes; offsets native, or divided too under rescale_offsets."""
    from bonai_amd import kernels as K
    from bonai_amd.dataset import BonaiDataset
    from bonai_amd.loft.roi import _view_rois
    f = _dataset_files(tmp_path, (SRC,))
    ds = BonaiDataset(f, str(tmp_path), test_mode=True, resize=dict(img_scale=(128, 128), keep_ratio=True))
    (_, data), = list(ds.test_batches())
    meta = data['img_metas'][0][0]
    assert meta['ori_shape'] == (SRC, SRC, 3) and meta['img_shape'] == (128, 128, 3) and meta['pad_shape'] == (128, 128, 3)
    native = torch.from_numpy(RR.image_prep(_rgb(tmp_path, ds.data_infos[0]), (128, 128), (128, 128), 0, True, MEAN, STD))[None].cuda()
    assert torch.equal(data['img'][0], native)
    nmeta = [dict(img_shape=(128, 128, 3), pad_shape=(128, 128, 3), ori_shape=(128, 128, 3), scale_factor=np.ones(4, np.float32), flip=False)]
    cfg = model.roi_head.test_cfg
    with torch.no_grad():
        x = model.extract_feat(native)
        props = model.rpn_head.simple_test_rpn(x, nmeta)
        nb, nl, _, _ = model.roi_head.simple_test_device(x, props, nmeta)
        sf = torch.from_numpy(meta['scale_factor']).cuda()
        # the result stage's RoIs are the divided boxes multiplied back (test_mixins.py:222-223: det_bboxes[:, :4] * scale_factor),
        # which is not the undivided box in its last bit: the native heads run on those
        back = ((nb[:, :4] / sf) * sf).contiguous()
        rois = _view_rois(back, None, None)
        logits = model.roi_head._mask_logits(x, rois, nl).float()
        noff = model.roi_head.offset_head.get_offsets_device(model.roi_head._offset_forward(x, rois), back).float()
        plain = model(img=data['img'], img_metas=data['img_metas'], return_loss=False, rescale=True)
        cfg['rescale_offsets'] = True
        try:
            scaled = model(img=data['img'], img_metas=data['img_metas'], return_loss=False, rescale=True)
        finally:
            cfg.pop('rescale_offsets')
    assert nb.shape[0] > 0 and torch.allclose(back, nb[:, :4], rtol=1e-6, atol=0) and (meta['scale_factor'] == np.float32(128 / 96)).all()
    boxes = nb[:, :4] / sf
    for res in (plain, scaled):
        assert np.array_equal(res[0][0][:, :4], boxes.cpu().numpy()) and np.array_equal(res[0][0][:, 4], nb[:, 4].cpu().numpy())
        want = K.mask_paste(logits, (back / sf).contiguous(), SRC, SRC, cfg.mask_thr_binary).bool().cpu().numpy()
        assert len(res[1][0]) == want.shape[0] and all(np.array_equal(a, b) for a, b in zip(res[1][0], want))
    assert np.array_equal(plain[2], noff.cpu().numpy())
    assert np.array_equal(scaled[2], (noff / sf[:2]).cpu().numpy()) and not np.array_equal(scaled[2], plain[2])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_what_is_not_built_is_refused_by_name(tmp_path, model):
    from bonai_amd import data as D, tta
    from bonai_amd.config import Config
    from bonai_amd.dataset import BonaiDataset
    from bonai_amd.scene import SceneDetector
    f = _dataset_files(tmp_path)
    rs = dict(img_scale=(128, 128))
    # multi-scale test views, and a resized view together with flips or rotations
    with pytest.raises(NotImplementedError, match='multi-scale test views'):
        BonaiDataset(f, str(tmp_path), test_mode=True, resize=dict(img_scale=[(64, 64), (128, 128)], multiscale_mode='value'))
    with pytest.raises(NotImplementedError, match='multi-scale test views'):
        tta.resize_from_pipeline([dict(type='MultiScaleFlipAug', img_scale=[(64, 64), (128, 128)], flip=False, transforms=[])], (96, 96))
    with pytest.raises(NotImplementedError, match='flips or rotations'):
        tta.resize_from_pipeline([dict(type='MultiScaleFlipAug', img_scale=(128, 128), flip=True, transforms=[])], (96, 96))
    with pytest.raises(NotImplementedError, match='test_views'):
        BonaiDataset(f, str(tmp_path), test_mode=True, resize=rs, test_views=[None, 'horizontal'], img_scale=(96, 96))
    got = tta.resize_from_pipeline([dict(type='MultiScaleFlipAug', img_scale=(128, 128), flip=False,
                                         transforms=[dict(type='Resize', keep_ratio=True), dict(type='Pad', size_divisor=64)])], (96, 96))
    assert got == dict(resize=dict(img_scale=(128, 128), keep_ratio=True), pad_divisor=64)
    assert tta.resize_from_pipeline([dict(type='MultiScaleFlipAug', img_scale=(96, 96), flip=True, transforms=[])], (96, 96)) is None
    # Resize inside SceneDetector
    cfg = Config(dict(data=dict(test=dict(img_scale=(96, 96), pipeline=[dict(type='MultiScaleFlipAug', img_scale=(128, 128), flip=False,
                                                                                 transforms=[])]))))
    with pytest.raises(NotImplementedError, match='Resize inside SceneDetector'):
        SceneDetector(model, tile=128, overlap=64, cfg=cfg)
    # per-sample scale draws: a batch whose samples carry different geometries
    ds = BonaiDataset(f, str(tmp_path), flip_ratio=0.0, resize=dict(img_scale=[(64, 64), (128, 128)], multiscale_mode='value'))
    with pytest.raises(NotImplementedError, match='per-sample scale draws'):
        D.to_device_batch([ds._train_sample(0, (64, 64)), ds._train_sample(1, (128, 128))])
    # mixed source sizes in training: at construction from the annotation file, and by name when a file lies about its size
    with pytest.raises(NotImplementedError, match='mixed source sizes'):
        BonaiDataset(_dataset_files(tmp_path, (SRC, 64), 'mixed.json'), str(tmp_path), resize=rs)
    ds.data_infos[1] = dict(ds.data_infos[1], filename='tile_1_64.png')
    with pytest.raises(NotImplementedError, match='tile_1_64.png'):
        ds._train_sample(1, (128, 128))
    # backend='pillow' and other interpolations
    with pytest.raises(NotImplementedError, match='pillow'):
        BonaiDataset(f, str(tmp_path), resize=dict(rs, backend='pillow'))
    with pytest.raises(NotImplementedError, match='bilinear'):
        BonaiDataset(f, str(tmp_path), resize=dict(rs, interpolation='nearest'))
    # a padded side that is a multiple of 32 but not of 64
    with pytest.raises(NotImplementedError, match='pad_divisor=64'):
        BonaiDataset(f, str(tmp_path), resize=dict(img_scale=(160, 160)))
