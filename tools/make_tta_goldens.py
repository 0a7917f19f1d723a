#!/usr/bin/env python
"""Writes the test-time-augmentation fixtures from the reference's own python:

  tests/golden/tta_ops.npz   seeded inputs and the outputs of bbox_mapping / bbox_mapping_back (mmdet/core/bbox/transforms.py:30-51)
                             for none / horizontal / vertical on a 64 x 96 shape, merge_aug_bboxes, merge_aug_masks and
                             merge_aug_proposals (mmdet/core/post_processing/merge_augs.py) for V = 2 and 3
  tests/golden/tta_256.npz   the reference model's aug_test -- m(img=[3 views], img_metas=[...], return_loss=False, rescale=True) -- on
                             the seeded 256^2 tile of oracle/ref_harness/make_goldens.py::e2e_test with synthetic weights, views
                             none / horizontal / vertical built with np.flip: the fields of e2e_test_256.npz without ``offsets``
                             (StandardRoIHead.aug_test returns none)

    BONAI_REFERENCE=/path/to/reference python tools/make_tta_goldens.py [--ops-only]

Runs on the CPU, where a checkout of the reference is at hand; the tests only read the fixtures.  mmcv is not installed:
oracle/ref_harness/mmcv_stub.py supplies the stand-ins and routes mmcv.ops.nms to the C oracle.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'ref_harness'))
GOLD = os.path.join(ROOT, 'tests', 'golden')
SHAPE = (64, 96, 3)
DIRS = (None, 'horizontal', 'vertical')


def _meta(d, shape=SHAPE):
    return dict(img_shape=shape, ori_shape=shape, pad_shape=shape, scale_factor=np.array([1., 1., 1., 1.], dtype=np.float32),
                flip=d is not None, flip_direction=d)


def _boxes(rng, n, h, w):
    x, y = rng.uniform(-4, w - 2, n), rng.uniform(-4, h - 2, n)
    b = np.stack([x, y, x + rng.uniform(0.5, w / 2, n), y + rng.uniform(0.5, h / 2, n)], 1).astype(np.float32)
    b[:4] = [[0, 0, w, h], [0, 0, 0, 0], [w - 3, h - 5, w, h], [10.5, 20.25, 10.5, 31]]      # borders, zero area
    return b


def ops():
    from mmdet.core.bbox.transforms import bbox_mapping, bbox_mapping_back
    from mmdet.core.post_processing.merge_augs import merge_aug_bboxes, merge_aug_masks, merge_aug_proposals
    from bonai_amd.config import Config
    rng = np.random.RandomState(31)
    h, w = SHAPE[:2]
    out = dict(img_shape=np.array(SHAPE, dtype=np.int64))
    boxes = torch.from_numpy(_boxes(rng, 40, h, w))
    out['boxes'] = boxes.numpy()
    for d in DIRS:
        m = _meta(d)
        out[f'mapping_{d}'] = bbox_mapping(boxes, m['img_shape'], m['scale_factor'], m['flip'], m['flip_direction'] or 'horizontal').numpy()
        out[f'mapping_back_{d}'] = bbox_mapping_back(boxes, m['img_shape'], m['scale_factor'], m['flip'],
                                                     m['flip_direction'] or 'horizontal').numpy()
    for V in (2, 3):
        metas = [[_meta(d)] for d in DIRS[:V]]
        ab = [torch.from_numpy(_boxes(rng, 33, h, w)) for _ in range(V)]           # C = 1: [n, 4]
        sc = [torch.softmax(torch.from_numpy(rng.randn(33, 2).astype(np.float32) * 3), 1) for _ in range(V)]
        mb, ms = merge_aug_bboxes(ab, sc, metas, None)
        out[f'bboxes_in_{V}'], out[f'scores_in_{V}'] = np.stack([a.numpy() for a in ab]), np.stack([s.numpy() for s in sc])
        out[f'bboxes_out_{V}'], out[f'scores_out_{V}'] = mb.numpy(), ms.numpy()
        am = [torch.from_numpy(rng.randn(9, 1, 28, 28).astype(np.float32) * 3).sigmoid().numpy() for _ in range(V)]
        out[f'masks_in_{V}'] = np.stack(am)
        out[f'masks_out_{V}'] = np.asarray(merge_aug_masks(am, metas, None), dtype=np.float32)
        props = []
        for _ in range(V):
            p = np.concatenate([_boxes(rng, 120, h, w), np.round(rng.uniform(0.01, 1, (120, 1)), 3).astype(np.float32)], 1)
            props.append(torch.from_numpy(p[np.argsort(-p[:, 4], kind='stable')].copy()))
        cfg = Config(dict(nms_thr=0.7, max_num=100))
        out[f'props_in_{V}'] = np.stack([p.numpy() for p in props])
        out[f'props_out_{V}'] = merge_aug_proposals(props, [_meta(d) for d in DIRS[:V]], cfg).numpy()
    out['rpn_nms_thr'], out['rpn_max_num'] = np.float32(0.7), np.int64(100)
    path = os.path.join(GOLD, 'tta_ops.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


def e2e(size=256):
    from bonai_amd.config import Config
    from bonai_amd.synth import make_batch
    from mmdet.models import build_detector
    from oracle.synth_weights import synth_state_dict
    ref = os.environ.get('BONAI_REFERENCE', '/root/reference')
    cfg = Config.fromfile(os.path.join(ref, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    cfg.model.pretrained = None
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict(synth_state_dict(m.state_dict()))
    m.eval()
    data = make_batch(1, size, 4)
    img = data['img'].numpy()
    views = [img, np.flip(img, 3).copy(), np.flip(img, 2).copy()]
    metas = [[dict(data['img_metas'][0], flip=d is not None, flip_direction=d)] for d in DIRS]
    with torch.no_grad():
        res = m(img=[torch.from_numpy(v) for v in views], img_metas=metas, return_loss=False, rescale=True)
    assert len(res) == 2, 'StandardRoIHead.aug_test returns (bbox_results, segm_results): no offsets'
    bbox_results, segm_results = res
    det = bbox_results[0]
    masks = np.stack(segm_results[0]) if len(segm_results[0]) else np.zeros((0, size, size), bool)
    out = dict(det=det.astype(np.float32), mask_area=masks.reshape(masks.shape[0], -1).sum(1).astype(np.int64),
               mask_rowsum=masks.sum(2).astype(np.int32)[:64], meta=np.array([size]))
    path = os.path.join(GOLD, f'tta_{size}.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes; dets', det.shape, 'top', det[:2], 'areas', out['mask_area'][:5])


def main():
    import mmcv_stub
    mmcv_stub.install()
    # the stub registers the submodule mmcv.ops.nms after the function of the same name, which shadows it for
    # `from mmcv.ops import nms` (merge_augs.py:3); the function -- the C oracle's -- is put back
    from oracle import cops
    sys.modules['mmcv.ops'].nms = cops.nms
    ops()
    if '--ops-only' not in sys.argv:
        e2e()


if __name__ == '__main__':
    main()
