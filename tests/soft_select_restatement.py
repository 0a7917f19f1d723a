"""numpy restatement of the per-image multiclass_nms with soft-NMS (mmdet/core/post_processing/bbox_nms.py:5-69 with mmcv-1.0.5's
batched_nms and soft_nms), written as loops over candidates: the statement kernels.multiclass_soft_nms_batched is held to, image by
image.  Every floating-point step is one fp32 operation, in the order of the tensor expressions and of oracle/loft_oracle.c:

  candidates   (row, class) with score > score_thr, strictly, in ascending flat index row * C + class -- `valid.nonzero()`'s order
  shift        class * (max over the candidates' coordinates + 1), added to the four coordinates; class_agnostic: none
  selection    soft_nms_sim (tests/test_select_forms_cpu.py) on the shifted boxes: in-place max selection, first position wins a tie,
               decay naive / linear, the drop with its hole / filler arrangement
  cut          the first max_num selections, when max_num > 0
  output       the UNSHIFTED box of each selection and its decayed score

Also the batches the CPU and the GPU tests share (``batch``, ``NAMES``) and the hand-derived cases (``hand_cases``)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import det_select_restatement as D  # noqa: E402
from test_select_forms_cpu import soft_nms_sim  # noqa: E402

F = np.float32
SIGMA, MIN_SCORE = 0.5, 1e-3                            # kernels.soft_nms's defaults


def candidates(bboxes, scores, score_thr):
    """-> [(score, flat, box, label)] in ascending flat index."""
    bboxes, scores = np.asarray(bboxes, F), np.asarray(scores, F)
    R, C = scores.shape[0], scores.shape[1] - 1
    cand = []
    for r in range(R):
        for c in range(C):
            if scores[r, c] > F(score_thr):
                box = bboxes[r, 4 * c:4 * c + 4] if bboxes.shape[1] > 4 else bboxes[r]
                cand.append((scores[r, c], r * C + c, box, c))
    return cand


def multiclass_soft_nms(bboxes, scores, score_thr, iou_thr, method='linear', max_num=-1, class_agnostic=False, sigma=SIGMA,
                        min_score=MIN_SCORE, info=None):
    """bboxes fp32 [R, 4C] or [R, 4], scores fp32 [R, C+1] -> (dets fp32 [n,5], labels int64 [n]).  info (a dict, optional) receives
    candidates, selections (before the cut), drop_rounds and fillers of the selection."""
    cand = candidates(bboxes, scores, score_thr)
    if info is not None:
        info.update(candidates=len(cand), selections=0, drop_rounds=0, fillers=0)
    if not cand:
        return np.zeros((0, 5), F), np.zeros((0,), np.int64)
    boxes = np.stack([box for _, _, box, _ in cand]).astype(F)
    if class_agnostic:
        shifted = boxes
    else:
        biggest = boxes.max()                                              # numpy's max propagates NaN, as torch's does
        with np.errstate(invalid='ignore', over='ignore'):
            shifted = np.stack([box + F(c) * (biggest + F(1)) for _, _, box, c in cand]).astype(F)
    sc = np.array([s for s, _, _, _ in cand], F)
    with np.errstate(divide='ignore', invalid='ignore'):
        sim = soft_nms_sim(shifted, sc, iou_thr, sigma, min_score, method, F)
    inds, decayed = sim['inds'], sim['dets'][:, 4]
    if info is not None:
        info.update(selections=len(inds), drop_rounds=sim['drop_rounds'], fillers=sim['fillers'])
    if max_num > 0:
        inds, decayed = inds[:max_num], decayed[:max_num]
    dets = np.concatenate([boxes[inds], decayed[:, None].astype(F)], 1).astype(F).reshape(-1, 5)
    return dets, np.array([cand[i][3] for i in inds], np.int64)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
def hand_cases():
    """name -> (bboxes, scores, score_thr, iou_thr, method, max_num, rows of dets, labels), every answer derived by hand."""
    A, Bx, Cx = [0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]
    return {
        # one row, two classes, one score: flat index 0 (class 0) before flat index 1 (class 1)
        'equal_scores_two_classes_flat_order': ([A], [[.5, .5, 0]], .05, .5, 'linear', -1, [A + [.5], A + [.5]], [0, 1]),
        # C = 2, shared boxes; flat 0 (row 0, class 0, .5), 1 (row 0, class 1, .5), 2 (row 1, class 0, .5), 3 (row 1, class 1, .7).  The
        # largest coordinate is 30, so class 1 lives 31 further out and nothing overlaps.  Slot 0 takes flat 3 and SWAPS it with flat 0:
        # the positions now hold 3 | 1 2 0, and the three ties leave in that order -- not in the order a sort would give them
        'equal_scores_after_a_swap': ([A, Bx], [[.5, .5, 0], [.5, .7, 0]], .05, .5, 'linear', -1,
                                      [Bx + [.7], A + [.5], Bx + [.5], A + [.5]], [1, 1, 0, 0]),
        # the same box twice: IoU exactly 1, linear weight 1 - 1 = 0, score 0 < min_score: dropped.  Bx is disjoint and stays
        'exact_duplicate_linear_is_dropped': ([A, A, Bx], [[.9, 0], [.8, 0], [.4, 0]], .05, .5, 'linear', -1, [A + [.9], Bx + [.4]], [0, 0]),
        # [0,0,2,1] inside [0,0,2,2]: IoU 2 / 4 = 0.5 >= 0.5: linear weight 0.5, and fp32(0.8) * 0.5 is fp32(0.4) exactly; naive drops it
        'half_overlap_linear_halves': ([[0, 0, 2, 2], [0, 0, 2, 1]], [[.9, 0], [.8, 0]], .05, .5, 'linear', -1,
                                       [[0, 0, 2, 2, .9], [0, 0, 2, 1, .4]], [0, 0]),
        'half_overlap_naive_drops': ([[0, 0, 2, 2], [0, 0, 2, 1]], [[.9, 0], [.8, 0]], .05, .5, 'naive', -1, [[0, 0, 2, 2, .9]], [0]),
        # three disjoint boxes, two wanted: the cut lands inside the selection
        'cut_inside_the_selection': ([A, Bx, Cx], [[.5, 0], [.6, 0], [.4, 0]], .05, .5, 'linear', 2, [Bx + [.6], A + [.5]], [0, 0]),
    }


CAPACITY = 4096                                         # kernels.SOFT_NMS_LDS_CAPACITY (asserted equal in the tests)


def _empty(C, box_cols):
    return np.zeros((0, box_cols), F), np.zeros((0, C + 1), F)


@functools.lru_cache(maxsize=None)
def batch(name):
    """-> (images [(bboxes, scores)], score_thr, iou_thr, max_per_img)."""
    if name.startswith('three_'):                      # 0, 37 and 300 rows; the cut lands inside the selections of the last two
        C, box_cols = {'three_c1': (1, 4), 'three_c3_per_class': (3, 12), 'three_c3_shared_box': (3, 4)}[name]
        return [_empty(C, box_cols), D.random_image(37, C, box_cols, 37 + C), D.random_image(300, C, box_cols, 300 + C)], 0.05, 0.5, 10
    if name == 'one_image_below_thr':
        b, s = D.random_image(50, 3, 12, 5)
        return [D.random_image(40, 3, 12, 6), (b, s * F(0.04)), D.random_image(60, 3, 12, 7)], 0.05, 0.5, 400
    if name == 'one_row':
        return [D.random_image(1, 1, 4, 8)], 0.0, 0.5, 10
    if name == 'all_empty':
        return [_empty(2, 8)] * 3, 0.05, 0.5, 10
    if name == 'sixteen_small':
        return [D.random_image(3 + 2 * i, 2, 8, 20 + i) for i in range(16)], 0.05, 0.5, 30
    if name == 'ties_sixteenths':                      # scores quantised to 1/16: ties everywhere
        out = []
        for rows, seed in ((90, 31), (200, 32)):
            b, s = D.random_image(rows, 2, 8, seed)
            out.append((b, (np.floor(s * 16) / 16).astype(F)))
        return out, 0.05, 0.5, 150
    if name == 'clustered_5000_duplicates':            # 5000 rows > capacity: the workspace form, stopped early, next to a small image
        b, s = D.clustered_image()
        b = b.copy()
        b[100:160] = b[40:100]                         # exact duplicate rows: linear decays them to 0
        return [D.random_image(20, 1, 4, 3), (b, s)], 0.05, 0.5, 100
    if name == 'capacity_rows':
        return [D.random_image(CAPACITY, 1, 4, 41)], 0.05, 0.5, 50
    if name == 'capacity_plus_one_rows':
        return [D.random_image(CAPACITY + 1, 1, 4, 42)], 0.05, 0.5, 50
    raise KeyError(name)


NAMES = ['three_c1', 'three_c3_per_class', 'three_c3_shared_box', 'one_image_below_thr', 'one_row', 'all_empty', 'sixteen_small',
         'ties_sixteenths', 'clustered_5000_duplicates', 'capacity_rows', 'capacity_plus_one_rows']


def classes(name):
    return batch(name)[0][0][1].shape[1] - 1


def variants():
    """(name, class_agnostic): every batch, and the C > 1 ones also class-agnostic."""
    return [(n, a) for n in NAMES for a in ((False, True) if classes(n) > 1 else (False,))]


@functools.lru_cache(maxsize=None)
def want(name, method, class_agnostic=False):
    """The restatement's (dets, labels, info) per image of a batch; computed once, shared, never modified."""
    images, score_thr, iou_thr, k = batch(name)
    out = []
    for b, s in images:
        info = {}
        d, l = multiclass_soft_nms(b, s, score_thr, iou_thr, method, k, class_agnostic, info=info)
        d.setflags(write=False)
        l.setflags(write=False)
        out.append((d, l, info))
    return out
