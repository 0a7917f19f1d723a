"""CPU: tests/det_select_restatement.py -- the statement the GPU tests hold kernels.multiclass_nms_batched to -- against answers
derived by hand and against oracle.ops_ref.multiclass_nms, exactly; and SceneDetector's ``batch`` argument."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import det_select_restatement as D  # noqa: E402

from oracle import ops_ref  # noqa: E402

HAND = D.hand_cases()


def _oracle(bboxes, scores, score_thr, iou_thr, predicate, max_num):
    dets, labels = ops_ref.multiclass_nms(torch.from_numpy(np.asarray(bboxes, np.float32)), torch.from_numpy(np.asarray(scores, np.float32)),
                                          score_thr, dict(type='nms', iou_threshold=iou_thr, predicate=predicate), max_num)
    return dets.numpy(), labels.numpy()


@pytest.mark.parametrize('predicate', ['device', 'cpu'])
@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(name, predicate):
    bboxes, scores, score_thr, iou_thr, max_num, want = HAND[name]
    dets, labels = D.multiclass_nms(bboxes, scores, score_thr, iou_thr, predicate, max_num)
    assert dets.dtype == np.float32 and labels.dtype == np.int64
    assert np.array_equal(dets, np.array(want[predicate][0], np.float32).reshape(-1, 5)) and labels.tolist() == want[predicate][1]
    od, ol = _oracle(bboxes, scores, score_thr, iou_thr, predicate, max_num)
    assert np.array_equal(od, dets) and np.array_equal(ol, labels)


def test_the_two_predicates_differ_only_at_the_threshold():
    want = HAND['iou_equal_to_thr'][5]
    assert want['device'] != want['cpu']
    assert all(HAND[n][5]['device'] == HAND[n][5]['cpu'] for n in HAND if n != 'iou_equal_to_thr')


@pytest.mark.parametrize('predicate', ['device', 'cpu'])
@pytest.mark.parametrize('rows, C, box_cols, max_num', [(0, 1, 4, 10), (37, 1, 4, 10), (300, 1, 4, 10), (37, 3, 12, 10), (300, 3, 12, 10),
                                                       (300, 3, 4, 10), (300, 3, 12, -1), (1, 1, 4, 10)])
def test_restatement_equals_the_oracle(rows, C, box_cols, max_num, predicate):
    bboxes, scores = D.random_image(rows, C, box_cols, seed=rows + C)
    dets, labels = D.multiclass_nms(bboxes, scores, 0.05, 0.5, predicate, max_num)
    od, ol = _oracle(bboxes, scores, 0.05, 0.5, predicate, max_num)
    assert np.array_equal(od.view(np.int32), dets.view(np.int32)) and np.array_equal(ol, labels)
    if rows == 300:                                     # the inputs do what they are for: suppression, ties, and a cut that bites
        full, _ = D.multiclass_nms(bboxes, scores, 0.05, 0.5, predicate, -1)
        assert 10 < full.shape[0] < 0.8 * rows * C and len(set(full[:, 4].tolist())) < full.shape[0]
        assert dets.shape[0] == (10 if max_num > 0 else full.shape[0])


def test_all_scores_below_the_threshold():
    bboxes, scores = D.random_image(20, 3, 12, seed=4)
    dets, labels = D.multiclass_nms(bboxes, scores * np.float32(0.04), 0.05, 0.5)
    assert dets.shape == (0, 5) and labels.shape == (0,)


def test_clustered_segment():
    bboxes, scores = D.clustered_image()
    dets, labels = D.multiclass_nms(bboxes, scores, 0.05, 0.5, 'device', -1)
    od, ol = _oracle(bboxes, scores, 0.05, 0.5, 'device', -1)
    assert 30 <= dets.shape[0] < 500                    # 5000 candidates, most suppressed
    assert np.array_equal(od.view(np.int32), dets.view(np.int32)) and np.array_equal(ol, labels)


# ---------------------------------------------------------------------------------------------------------------- SceneDetector(batch=)
class _Stub:
    """What SceneDetector's constructor reads of a model: roi_head.test_cfg and roi_head.with_mask."""

    def __init__(self, nms_type='nms'):
        from bonai_amd.config import ConfigDict
        self.roi_head = type('Roi', (), {})()
        self.roi_head.with_mask = True
        self.roi_head.test_cfg = ConfigDict(score_thr=0.05, nms=ConfigDict(type=nms_type, iou_threshold=0.5), max_per_img=100,
                                            mask_thr_binary=0.5)


@pytest.mark.parametrize('bad', [0, 17, -1, 2.0, 1.5, True, None, '2'])
def test_scene_detector_refuses_a_batch_out_of_range(bad):
    from bonai_amd.scene import SceneDetector
    with pytest.raises(ValueError, match='batch'):
        SceneDetector(_Stub(), tile=64, overlap=32, batch=bad)


def test_scene_detector_takes_every_batch_in_range():
    from bonai_amd.scene import PREP_CHUNK, SceneDetector
    assert PREP_CHUNK == 16
    assert SceneDetector(_Stub(), tile=64, overlap=32).batch == 1
    for b in (1, 2, 8, 16, np.int64(4)):
        assert SceneDetector(_Stub(), tile=64, overlap=32, batch=b).batch == int(b)


def test_scene_detector_refuses_soft_nms_in_batches():
    from bonai_amd.scene import SceneDetector
    with pytest.raises(ValueError, match='batch=1'):
        SceneDetector(_Stub('soft_nms'), tile=64, overlap=32, batch=2)
    assert SceneDetector(_Stub('soft_nms'), tile=64, overlap=32, batch=1).batch == 1
