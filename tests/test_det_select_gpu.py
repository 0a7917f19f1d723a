"""GPU: kernels.multiclass_nms_batched (bonai_amd/csrc/detect.hip) against the loop restatement of tests/det_select_restatement.py
and against oracle.ops_ref.multiclass_nms, image by image, and against LoftRoIHead.multiclass_nms -- the per-image device path it
stands in for -- on the same device inputs.  Detections, labels, counts, the zero padding and the RoIs: exactly."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import det_select_restatement as D  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = D.hand_cases()
NONE = (np.zeros((0, 5), np.float32), np.zeros((0,), np.int64))      # an image without rows: the per-image forms cannot view [0, 4C]


def _empty(C, box_cols):
    return np.zeros((0, box_cols), np.float32), np.zeros((0, C + 1), np.float32)


@functools.lru_cache(maxsize=None)
def _batch(name):
    """-> (images [(bboxes, scores)], score_thr, iou_thr, max_per_img)."""
    if name.startswith('three_'):                      # 0, 37 and 300 rows
        C, box_cols = {'three_c1': (1, 4), 'three_c3_per_class': (3, 12), 'three_c3_shared_box': (3, 4)}[name]
        return [_empty(C, box_cols), D.random_image(37, C, box_cols, 37 + C), D.random_image(300, C, box_cols, 300 + C)], 0.05, 0.5, 10
    if name == 'one_image_below_thr':
        b, s = D.random_image(50, 3, 12, 5)
        return [D.random_image(40, 3, 12, 6), (b, s * np.float32(0.04)), D.random_image(60, 3, 12, 7)], 0.05, 0.5, 100
    if name == 'one_row':
        return [D.random_image(1, 1, 4, 8)], 0.0, 0.5, 10
    if name == 'all_empty':
        return [_empty(2, 8)] * 3, 0.05, 0.5, 10
    if name == 'all_below_thr':
        return [(b, s * np.float32(0.04)) for b, s in (D.random_image(30, 1, 4, 1), D.random_image(5, 1, 4, 2))], 0.05, 0.5, 10
    if name == 'clustered_5000':
        return [D.random_image(20, 1, 4, 3), D.clustered_image()], 0.05, 0.5, 4096
    if name == 'many_rows_two_stage_topk':             # 3 x 11 000 > TOPK_MAX_SEGMENT: the selection in two stages
        b, s = D.random_image(11000, 3, 4, 10)
        s[:, :3] *= (np.arange(11000) % 50 == 0)[:, None]      # 220 rows above the threshold
        return [D.random_image(30, 3, 4, 11), (b, s)], 0.05, 0.5, 50
    bboxes, scores, score_thr, iou_thr, max_num, _ = HAND[name]          # in image 1 of 3
    bboxes, scores = np.asarray(bboxes, np.float32), np.asarray(scores, np.float32)
    C, cols = scores.shape[1] - 1, bboxes.shape[1]
    # (max_num = -1, "no cut", is not a max_per_img: 20 is more than a hand case has candidates)
    return [D.random_image(23, C, cols, 12), (bboxes, scores), D.random_image(9, C, cols, 13)], score_thr, iou_thr, max_num if max_num > 0 else 20


NAMES = ['three_c1', 'three_c3_per_class', 'three_c3_shared_box', 'one_image_below_thr', 'one_row', 'all_empty', 'all_below_thr',
         'clustered_5000', 'many_rows_two_stage_topk'] + sorted(HAND)


@functools.lru_cache(maxsize=None)
def _want(name, predicate):
    images, score_thr, iou_thr, k = _batch(name)
    return [D.multiclass_nms(b, s, score_thr, iou_thr, predicate, k) for b, s in images]


def _run(name, predicate, roi_off_on_device=False):
    from bonai_amd import kernels as K
    images, score_thr, iou_thr, k = _batch(name)
    bboxes = torch.from_numpy(np.concatenate([b for b, _ in images])).cuda()
    scores = torch.from_numpy(np.concatenate([s for _, s in images])).cuda()
    off = np.cumsum([0] + [b.shape[0] for b, _ in images]).tolist()
    cfg = dict(type='nms', iou_threshold=iou_thr, predicate=predicate)
    out = K.multiclass_nms_batched(bboxes, scores, torch.tensor(off).cuda() if roi_off_on_device else off, score_thr, cfg, k)
    return (bboxes, scores, off, cfg), out


def _check(name, want, out):
    images, _, _, k = _batch(name)
    dets, labels, counts, rois = out
    B = len(images)
    assert dets.shape == (B, k, 5) and dets.dtype == torch.float32 and labels.shape == (B, k) and labels.dtype == torch.int64
    assert counts.shape == (B,) and counts.dtype == torch.int64 and counts.is_cuda and rois.shape == (B * k, 5)
    dets, labels, rois = dets.cpu().numpy(), labels.cpu().numpy(), rois.cpu().numpy()
    assert counts.cpu().tolist() == [w[0].shape[0] for w in want]
    at = 0
    for b, (wd, wl) in enumerate(want):
        n = wd.shape[0]
        assert np.array_equal(dets[b, :n].view(np.int32), wd.view(np.int32)), (name, b)
        assert np.array_equal(labels[b, :n], wl), (name, b)
        assert not dets[b, n:].view(np.int32).any() and not labels[b, n:].any()                  # the padding: +0.0f and 0
        assert (rois[at:at + n, 0] == b).all() and np.array_equal(rois[at:at + n, 1:].view(np.int32), wd[:, :4].view(np.int32))
        at += n
    assert not rois[at:].view(np.int32).any()


@pytest.mark.parametrize('predicate', ['device', 'cpu'])
@pytest.mark.parametrize('name', NAMES)
def test_batched_equals_the_restatement(name, predicate):
    _, out = _run(name, predicate)
    _check(name, _want(name, predicate), out)
    if name in HAND:                                    # and the hand-derived answer itself, in image 1
        wd, wl = HAND[name][5][predicate]
        n = int(out[2][1])
        assert np.array_equal(out[0][1, :n].cpu().numpy(), np.array(wd, np.float32).reshape(-1, 5)) and out[1][1, :n].tolist() == wl


def test_the_inputs_reach_what_they_are_for():
    from bonai_amd import kernels as K
    n = [w[0].shape[0] for w in _want('three_c3_per_class', 'device')]
    images, thr, iou, _ = _batch('three_c3_per_class')
    full = D.multiclass_nms(*images[2], thr, iou, 'device', -1)[0].shape[0]
    assert n[0] == 0 and n[2] == 10 < full                                          # the cut takes effect on the 300-row image
    assert [w[0].shape[0] for w in _want('one_image_below_thr', 'device')][1] == 0
    c = _want('clustered_5000', 'device')[1][0].shape[0]
    assert 30 <= c < 500 and D.clustered_image()[0].shape[0] == 5000 > K.TOPK_MAX      # most of one long segment suppressed
    images, _, _, _ = _batch('many_rows_two_stage_topk')
    assert images[1][0].shape[0] * 3 > K.TOPK_MAX_SEGMENT


@pytest.mark.parametrize('name', ['three_c3_per_class', 'three_c3_shared_box', 'clustered_5000', 'equal_scores_lower_flat_index_first_across_classes'])
def test_batched_equals_the_oracle(name):
    from oracle import ops_ref
    images, score_thr, iou_thr, k = _batch(name)
    _, out = _run(name, 'device')
    want = []
    for b, s in images:
        d, l = ops_ref.multiclass_nms(torch.from_numpy(b), torch.from_numpy(s), score_thr, dict(type='nms', iou_threshold=iou_thr), k) \
            if b.shape[0] else NONE
        want.append((np.asarray(d), np.asarray(l)))
    _check(name, want, out)


@pytest.mark.parametrize('predicate', ['device', 'cpu'])
@pytest.mark.parametrize('name', ['three_c1', 'three_c3_per_class', 'three_c3_shared_box', 'clustered_5000', 'iou_equal_to_thr',
                                  'max_num_cuts_a_tie'])
def test_batched_equals_the_per_image_device_path(name, predicate):
    from bonai_amd.loft.roi import LoftRoIHead
    (bboxes, scores, off, cfg), out = _run(name, predicate, roi_off_on_device=True)
    k = _batch(name)[3]
    want = []
    for a, e in zip(off, off[1:]):
        if a == e:
            want.append(NONE)
            continue
        d, l = LoftRoIHead.multiclass_nms(None, bboxes[a:e], scores[a:e], _batch(name)[1], cfg, k)
        want.append((d.cpu().numpy(), l.cpu().numpy()))
    _check(name, want, out)


def test_refusals_by_name():
    from bonai_amd import kernels as K, lib as L
    b, s = (torch.from_numpy(a).cuda() for a in D.random_image(6, 2, 8, 1))
    ok = dict(type='nms', iou_threshold=0.5)
    with pytest.raises(L.LoftHipError, match='soft_nms'):
        K.multiclass_nms_batched(b, s, [0, 6], 0.05, dict(type='soft_nms', iou_threshold=0.5), 10)
    with pytest.raises(L.LoftHipError, match='class_agnostic'):
        K.multiclass_nms_batched(b, s, [0, 6], 0.05, dict(ok, class_agnostic=True), 10)
    for k in (0, -1, K.TOPK_MAX + 1):
        with pytest.raises(L.LoftHipError, match='max_per_img'):
            K.multiclass_nms_batched(b, s, [0, 6], 0.05, ok, k)
    with pytest.raises(L.LoftHipError, match='NMS_MAX_SEGMENT'):
        n = K.NMS_MAX_SEGMENT + 1
        K.multiclass_nms_batched(torch.zeros(n, 4, device='cuda'), torch.zeros(n, 2, device='cuda'), [0, n], 0.05, ok, 10)
    for off in ([0, 5], [1, 6], [0, 4, 3, 6], [6]):
        with pytest.raises(L.LoftHipError, match='roi_off'):
            K.multiclass_nms_batched(b, s, off, 0.05, ok, 10)
    with pytest.raises(L.LoftHipError, match='bboxes'):
        K.multiclass_nms_batched(b[:, :6].contiguous(), s, [0, 6], 0.05, ok, 10)
    with pytest.raises(L.LoftHipError):
        K.multiclass_nms_batched(b.cpu(), s.cpu(), [0, 6], 0.05, ok, 10)              # no host fall-back
