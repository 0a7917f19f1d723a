"""GPU: the headline config as it ships -- soft-NMS -- through the model in batches of tiles: LoftRoIHead.batch_test_device(...,
soft_nms_batched=True) and SceneDetector(batch=N, soft_nms_batched=True).  As in tests/test_scene_batch_gpu.py nothing is compared
ACROSS batch sizes (the convolution and FC kernel forms are chosen by problem size): batch_test_device is held to the per-image
pieces at the SAME batch, the scene's tile detections to batch_test_device group by group.  Everything exactly.

These checks share one model and are run by the single item of tests/test_soft_select_gpu.py (``check_all``), so that the whole
feature is one item of the suite; this file collects no test of its own."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_scene_batch_gpu import MEAN, STD, T, _build, _meta, _same, _scene_u8  # noqa: E402

pytestmark = pytest.mark.gpu


def _soft():
    m = _build(None)                                    # synthetic weights, max_per_img = 60, the NMS of the config: soft-NMS
    assert m.roi_head.test_cfg.nms['type'] == 'soft_nms' and m.roi_head.test_cfg.max_per_img == 60
    return m


def check_batch_test_device_equals_the_per_image_pieces_at_the_same_batch(soft, blank):
    from bonai_amd import kernels as K
    roi = soft.roi_head
    cfg = roi.test_cfg
    tiles = torch.stack([_scene_u8(T, T, 30 + k) for k in range(3)])
    if blank is not None:
        tiles[blank] = 0
    imgs = K.image_prep_d4(tiles.cuda(), [0] * 3, [False] * 3, MEAN, STD)
    metas = [_meta(T, T) for _ in range(3)]
    with torch.no_grad():
        x = soft.extract_feat(imgs)
        props, counts = soft.rpn_head.simple_test_rpn(x, metas)
        if blank is not None:                           # differing counts, padded proposal rows, one image without a RoI
            counts = torch.minimum(counts, torch.tensor([10 ** 6, 7, 0], device=counts.device))
        got = roi.batch_test_device(x, (props, counts), metas, soft_nms_batched=True)
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
    assert sum(per_image) > 0 and len(got) == 5, blank
    assert isinstance(got[4], np.ndarray) and got[4].dtype == np.int64 and got[4].tolist() == per_image
    assert _same(got[0], dets) and _same(got[1], labels) and _same(got[2], sel) and _same(got[3], offsets)
    if blank is not None:
        assert cnt[1:] == [7, 0] and per_image[2] == 0 and len(set(per_image)) > 1


def check_scene_tile_detections_in_batches_of_four_equal_batch_test_device_group_by_group(soft):
    """512 x 384 at tile 256, overlap 128: six tiles, a group of four and a group of two."""
    from bonai_amd import kernels as K
    from bonai_amd.scene import SceneDetector, tile_grid
    H, W = 384, 512
    origins = tile_grid(H, W, T, 128)
    assert len(origins) == 6
    scene = _scene_u8(H, W, 23).cuda()
    det = SceneDetector(soft, tile=T, overlap=128, batch=4, soft_nms_batched=True)
    got_origins, got = det.tile_detections(scene)
    assert got_origins.tolist() == origins.tolist() and len(got) == 6
    table = torch.from_numpy(origins).cuda()
    want = []
    with torch.no_grad():
        for g0 in (0, 4):
            imgs = K.scene_tile_prep(scene, table[g0:g0 + 4].contiguous(), (T, T), False, MEAN, STD)
            metas = [_meta(T, T) for _ in range(imgs.shape[0])]
            x = soft.extract_feat(imgs)
            d, l, m, o, n = soft.roi_head.batch_test_device(x, soft.rpn_head.simple_test_rpn(x, metas), metas, soft_nms_batched=True)
            ends = np.cumsum(n).tolist()
            want += [(d[e - k:e], l[e - k:e], m[e - k:e], o[e - k:e]) for e, k in zip(ends, n.tolist())]
    assert len(want) == 6 and sum(w[0].shape[0] for w in want) > 0
    for g, w in zip(got, want):
        assert len(g) == 4 and all(_same(a, b) for a, b in zip(g, w))
    res = det.run(scene)                                # and the merge runs on them
    assert 0 < len(res) <= sum(w[0].shape[0] for w in want)


def check_the_keyword_changes_nothing_for_hard_nms_and_the_refusal_stays_without_it(soft):
    from bonai_amd import lib as L
    roi = soft.roi_head
    imgs = torch.zeros(2, 3, T, T, device='cuda')
    metas = [_meta(T, T), _meta(T, T)]
    shipped = roi.test_cfg.nms
    with torch.no_grad():
        x = soft.extract_feat(imgs)
        props = soft.rpn_head.simple_test_rpn(x, metas)
        for kw in ({}, {'soft_nms_batched': False}):
            with pytest.raises(L.LoftHipError, match='soft_nms'):
                roi.batch_test_device(x, props, metas, **kw)
        roi.test_cfg.nms = type(shipped)(type='nms', iou_threshold=0.5)
        try:
            a = roi.batch_test_device(x, props, metas)
            b = roi.batch_test_device(x, props, metas, soft_nms_batched=True)
        finally:
            roi.test_cfg.nms = shipped
        assert all(_same(p, q) for p, q in zip(a[:4], b[:4])) and a[4].tolist() == b[4].tolist()


def check_all():
    soft = _soft()
    for blank in (None, 1):
        check_batch_test_device_equals_the_per_image_pieces_at_the_same_batch(soft, blank)
    check_scene_tile_detections_in_batches_of_four_equal_batch_test_device_group_by_group(soft)
    check_the_keyword_changes_nothing_for_hard_nms_and_the_refusal_stays_without_it(soft)
