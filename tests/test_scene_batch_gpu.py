"""GPU: tiles through the model in batches (LoftRoIHead.batch_test_device, SceneDetector(batch=N)).  The convolution and FC kernel
forms are chosen by problem size, so nothing is compared ACROSS batch sizes: batch_test_device is held to a reference assembled here
from the existing per-image pieces at the SAME batch, and the scene to the restatement's merge of detections obtained group by
group.  Everything exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
T = 256


def _scene_u8(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(H, W, 3, generator=g) * 58 + 120).clamp(0, 255).to(torch.uint8)


def _build(nms):
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    cfg.test_cfg.rcnn.max_per_img = 60           # as tests/test_scene_gpu.py: the synthetic weights fill any limit
    if nms is not None:
        cfg.test_cfg.rcnn.nms = nms
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    return m.cuda().eval()


@pytest.fixture(scope='module')
def model():
    """The headline config with the NMS a batch can run: it ships soft-NMS, which is sequential per image."""
    return _build(dict(type='nms', iou_threshold=0.5))


def _meta(h, w):
    return dict(img_shape=(h, w, 3), pad_shape=(h, w, 3), ori_shape=(h, w, 3), scale_factor=np.ones(4, np.float32), flip=False)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize('blank', [None, 1])
def test_batch_test_device_equals_the_per_image_pieces_at_the_same_batch(model, blank):
    from bonai_amd import kernels as K
    roi = model.roi_head
    cfg = roi.test_cfg
    tiles = torch.stack([_scene_u8(T, T, 30 + k) for k in range(3)])
    if blank is not None:
        tiles[blank] = 0                                                # an image whose counts differ from the others'
    imgs = K.image_prep_d4(tiles.cuda(), [0] * 3, [False] * 3, MEAN, STD)
    metas = [_meta(T, T) for _ in range(3)]
    with torch.no_grad():
        x = model.extract_feat(imgs)
        props, counts = model.rpn_head.simple_test_rpn(x, metas)
        if blank is not None:
            # the synthetic weights fill every limit, on a blank tile too: the proposal counts are cut here, so that the images'
            # counts differ, padded proposal rows must be dropped and one image has no RoI at all
            counts = torch.minimum(counts, torch.tensor([10 ** 6, 7, 0], device=counts.device))
        got = roi.batch_test_device(x, (props, counts), metas)
        cnt = counts.tolist()
        rois = torch.cat([torch.cat([props.new_full((n, 1), b), props[b, :n, :4]], 1) for b, n in enumerate(cnt)])
        cls_score, bbox_pred = roi.bbox_head(roi.bbox_roi_extractor(x[:roi.bbox_roi_extractor.num_inputs], rois))
        scores = torch.softmax(cls_score, dim=1)
        rr = rois[:, 1:].repeat_interleave(bbox_pred.shape[1] // 4, dim=0)
        bboxes = roi.bbox_head.bbox_coder.decode(rr, bbox_pred.reshape(-1, 4), max_shape=metas[0]['img_shape']).view(rois.shape[0], -1)
        dets, labels, at = [], [], 0
        for n in cnt:
            d, l = roi.multiclass_nms(bboxes[at:at + n], scores[at:at + n], cfg.score_thr, cfg.nms, cfg.max_per_img)
            dets.append(d), labels.append(l)
            at += n
        per_image = [d.shape[0] for d in dets]
        det_rois = torch.cat([torch.cat([d.new_full((d.shape[0], 1), b), d[:, :4]], 1) for b, d in enumerate(dets)])
        dets, labels = torch.cat(dets), torch.cat(labels)
        sel = roi._mask_logits(x, det_rois, labels).float()
        offsets = roi.offset_head.get_offsets_device(roi._offset_forward(x, det_rois), dets[:, :4].contiguous()).float()
    print(f'blank={blank}: proposals {cnt}, detections {per_image}')
    assert sum(per_image) > 0 and len(got) == 5
    assert isinstance(got[4], np.ndarray) and got[4].dtype == np.int64 and got[4].tolist() == per_image
    assert _same(got[0], dets) and _same(got[1], labels) and _same(got[2], sel) and _same(got[3], offsets)
    assert got[2].shape[1:] == (28, 28) and got[3].shape[1:] == (2,)
    if blank is not None:
        assert cnt[1:] == [7, 0] and per_image[2] == 0 and len(set(per_image)) > 1


def _restatement_merge(model, scene, origins, dets, H, W):
    from bonai_amd import kernels as K, rle as RL
    boxes, scores, logits, offsets, tiles = [], [], [], [], []
    for k, (d, l, m, o) in enumerate(dets):
        if d.shape[0]:
            boxes.append(d[:, :4].cpu().numpy()), scores.append(d[:, 4].cpu().numpy()), logits.append(m), offsets.append(o.cpu().numpy())
            tiles.append(np.full(d.shape[0], k, np.int32))
    boxes, scores, tiles, offsets = np.concatenate(boxes), np.concatenate(scores), np.concatenate(tiles), np.concatenate(offsets)
    logits = torch.cat(logits)
    thr = model.roi_head.test_cfg.mask_thr_binary
    scene_boxes = R.translate(boxes, tiles, origins)
    bitmaps = K.mask_paste(logits, torch.from_numpy(scene_boxes).cuda(), H, W, thr)
    keep = R.merge(bitmaps.bool().cpu().numpy(), scene_boxes, boxes, tiles, scores, origins, (T, T), H, W, 0.5, 2)
    roofs = RL.rle_encode_masks(bitmaps[torch.from_numpy(keep).cuda()])
    feet_boxes = torch.from_numpy(scene_boxes[keep]).cuda()
    feet = K.mask_paste_rle(logits[torch.from_numpy(keep).cuda()].contiguous(), feet_boxes, H, W, thr,
                            offsets=torch.from_numpy(offsets[keep]).cuda())
    return np.concatenate([scene_boxes, scores[:, None]], 1)[keep], tiles[keep], offsets[keep], roofs, feet, keep


def test_scene_in_batches_of_four_equals_the_restatement_merge(model):
    """A 640 x 384 scene has 4 x 2 = 8 tiles of 256 at overlap 128 -- two full groups of four; 512 x 384 has 3 x 2 = 6: a group of four
    and a short one of two."""
    from bonai_amd import kernels as K
    from bonai_amd.scene import SceneDetector, tile_grid
    assert len(tile_grid(384, 640, T, 128)) == 8
    H, W = 384, 512
    origins = tile_grid(H, W, T, 128)
    assert origins.tolist() == [[0, 0], [128, 0], [256, 0], [0, 128], [128, 128], [256, 128]] and len(origins) % 4 == 2
    scene = _scene_u8(H, W, 23).cuda()
    det = SceneDetector(model, tile=T, overlap=128, footprints=True, batch=4)
    res = det.run(scene)
    table = torch.from_numpy(origins).cuda()
    dets = []
    with torch.no_grad():                                                 # group by group, from the same pieces
        for g0 in (0, 4):
            imgs = K.scene_tile_prep(scene, table[g0:g0 + 4].contiguous(), (T, T), False, MEAN, STD)
            metas = [_meta(T, T) for _ in range(imgs.shape[0])]
            x = model.extract_feat(imgs)
            d, l, m, o, n = model.roi_head.batch_test_device(x, model.rpn_head.simple_test_rpn(x, metas), metas)
            ends = np.cumsum(n).tolist()
            dets += [(d[e - k:e], l[e - k:e], m[e - k:e], o[e - k:e]) for e, k in zip(ends, n.tolist())]
    assert len(dets) == 6
    bboxes, tiles, offsets, roofs, feet, keep = _restatement_merge(model, scene, origins.tolist(), dets, H, W)
    print(f'six tiles in groups of 4 + 2: {len(keep)} detections, {int(keep.sum())} kept, per tile {[int(d[0].shape[0]) for d in dets]}')
    assert len(set(tiles.tolist())) > 1 and 0 < keep.sum()
    assert np.array_equal(res.bboxes, bboxes) and np.array_equal(res.tiles, tiles) and np.array_equal(res.offsets, offsets)
    assert len(res.roofs) == len(roofs) and all(a == b for a, b in zip(res.roofs, roofs)) and roofs[0]['size'] == [H, W]
    assert len(res.footprints) == len(feet) and all(a == b for a, b in zip(res.footprints, feet))


def test_batch_one_is_the_per_tile_loop(model):
    """batch=1 after the change: tile_detections gives what the per-tile loop of
    tests/test_scene_gpu.py::test_four_tile_scene_equals_the_restatement_merge gives."""
    from bonai_amd import kernels as K
    from bonai_amd.scene import SceneDetector
    H, W = 384, 320
    scene = _scene_u8(H, W, 22).cuda()
    det = SceneDetector(model, tile=T, overlap=128)
    assert det.batch == 1
    origins, got = det.tile_detections(scene)
    assert origins.tolist() == [[0, 0], [64, 0], [0, 128], [64, 128]] and len(got) == 4
    for (x0, y0), g in zip(origins.tolist(), got):
        img = K.image_prep_d4(scene[y0:y0 + T, x0:x0 + T][None].contiguous(), [0], [False], MEAN, STD)
        with torch.no_grad():
            x = model.extract_feat(img)
            metas = [_meta(T, T)]
            want = model.roi_head.simple_test_device(x, model.rpn_head.simple_test_rpn(x, metas), metas)
        assert len(g) == 4 and all(_same(a, b) for a, b in zip(g, want))
    assert sum(g[0].shape[0] for g in got) > 0


def test_refusals(model):
    from bonai_amd import lib as L
    from bonai_amd.scene import SceneDetector
    soft = _build(None)                                                   # the headline config as it ships: soft-NMS
    assert soft.roi_head.test_cfg.nms['type'] == 'soft_nms'
    with pytest.raises(ValueError, match='batch=1'):
        SceneDetector(soft, tile=T, overlap=128, batch=2)
    assert SceneDetector(soft, tile=T, overlap=128, batch=1).batch == 1
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError, match='batch'):
            SceneDetector(model, tile=T, overlap=128, batch=bad)
    imgs = torch.zeros(2, 3, T, T, device='cuda')
    metas = [_meta(T, T), _meta(T, T)]
    with torch.no_grad():
        x = model.extract_feat(imgs)
        props = model.rpn_head.simple_test_rpn(x, metas)
        with pytest.raises(L.LoftHipError, match='soft_nms'):
            soft.roi_head.batch_test_device(x, props, metas)
        with pytest.raises(NotImplementedError, match='img_shape'):
            model.roi_head.batch_test_device(x, props, [_meta(T, T), _meta(T, T - 32)])
        with pytest.raises(NotImplementedError, match='scale_factor'):
            model.roi_head.batch_test_device(x, props, [_meta(T, T), dict(_meta(T, T), scale_factor=np.full(4, 2, np.float32))])
        cfg = model.roi_head.test_cfg
        cfg['paste_min_score'] = 0.4
        try:
            with pytest.raises(ValueError, match='paste_min_score'):
                model.roi_head.batch_test_device(x, props, metas)
        finally:
            cfg.pop('paste_min_score')
