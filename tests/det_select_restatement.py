"""numpy restatement of the per-image multiclass_nms (mmdet/core/post_processing/bbox_nms.py:5-69 with mmcv-1.0.5's batched_nms and
greedy NMS), written as loops over candidates: the statement kernels.multiclass_nms_batched is held to, image by image.  Every
floating-point step is one fp32 operation, in the order of the tensor expressions and of oracle/loft_oracle.c:

  candidates   (row, class) with score > score_thr, strictly, in ascending flat index row * C + class
  shift        class * (max over the candidates' coordinates + 1), added to the four coordinates for the IoU test only
  order        score descending, ties by ascending flat index (a stable sort)
  greedy       in that order a candidate is kept iff no KEPT one before it suppresses it: predicate 'device' inter > thr * union,
               predicate 'cpu' inter / union >= thr -- they differ at IoU == thr
  cut          the first max_num of the kept, when max_num > 0

Also the inputs the CPU and the GPU tests share (``hand_cases``, ``random_image``, ``clustered_image``)."""
import numpy as np

F = np.float32


def _suppressed(a, rest, thr, predicate):
    """a [4], rest [m,4] fp32 (shifted) -> bool [m]: a suppresses them."""
    left, right = np.maximum(a[0], rest[:, 0]), np.minimum(a[2], rest[:, 2])
    top, bottom = np.maximum(a[1], rest[:, 1]), np.minimum(a[3], rest[:, 3])
    w, h = np.maximum(right - left, F(0)), np.maximum(bottom - top, F(0))
    inter = w * h
    sa = (a[2] - a[0]) * (a[3] - a[1])
    sb = (rest[:, 2] - rest[:, 0]) * (rest[:, 3] - rest[:, 1])
    uni = sa + sb - inter
    if predicate == 'device':
        return inter > F(thr) * uni
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / uni >= F(thr)


def multiclass_nms(bboxes, scores, score_thr, iou_thr, predicate='device', max_num=-1):
    """bboxes fp32 [R, 4C] or [R, 4], scores fp32 [R, C+1] -> (dets fp32 [n,5], labels int64 [n])."""
    bboxes, scores = np.asarray(bboxes, F), np.asarray(scores, F)
    R, C = scores.shape[0], scores.shape[1] - 1
    cand = []                                           # (score, flat, box, label)
    for r in range(R):
        for c in range(C):
            if scores[r, c] > F(score_thr):
                box = bboxes[r, 4 * c:4 * c + 4] if bboxes.shape[1] > 4 else bboxes[r]
                cand.append((scores[r, c], r * C + c, box, c))
    if not cand:
        return np.zeros((0, 5), F), np.zeros((0,), np.int64)
    biggest = max(F(v) for _, _, box, _ in cand for v in box)
    cand.sort(key=lambda t: (-float(t[0]), t[1]))
    shifted = np.stack([box + F(c) * (biggest + F(1)) for _, _, box, c in cand]).astype(F)
    alive = np.ones(len(cand), bool)
    kept = []
    for i in range(len(cand)):
        if not alive[i]:
            continue
        kept.append(i)
        alive[i + 1:] &= ~_suppressed(shifted[i], shifted[i + 1:], iou_thr, predicate)
    if max_num > 0:
        kept = kept[:max_num]
    dets = np.array([list(cand[i][2]) + [cand[i][0]] for i in kept], F).reshape(-1, 5)
    return dets, np.array([cand[i][3] for i in kept], np.int64)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
def hand_cases():
    """name -> (bboxes, scores, score_thr, iou_thr, max_num, {predicate: (rows of dets, labels)}), every answer derived by hand."""
    A, Bx, Cx = [0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]
    both = lambda dets, labels: {'device': (dets, labels), 'cpu': (dets, labels)}      # noqa: E731
    return {
        # 0.25 is not > 0.25: only the second row is a candidate
        'score_equal_to_thr_is_dropped': ([A, Bx], [[.25, .75], [.5, .5]], .25, .5, -1, both([Bx + [.5]], [0])),
        # [0,0,2,1] inside [0,0,2,2]: inter 2, union 4, IoU exactly 0.5: 2 > 0.5 * 4 is false (kept), 2 / 4 >= 0.5 is true (suppressed)
        'iou_equal_to_thr': ([[0, 0, 2, 2], [0, 0, 2, 1]], [[.9, .1], [.8, .2]], .05, .5, -1,
                             {'device': ([[0, 0, 2, 2, .9], [0, 0, 2, 1, .8]], [0, 0]), 'cpu': ([[0, 0, 2, 2, .9]], [0])}),
        # C = 2, boxes [R, 4]: flat indices 0 (row 0, class 0, score .5), 1 (row 0, class 1, .5), 2 (row 1, class 0, .5), 3 (row 1,
        # class 1, .7).  Classes are shifted apart and A, Bx are disjoint: all kept; .7 first, then the three ties in flat order
        'equal_scores_lower_flat_index_first_across_classes': (
            [A, Bx], [[.5, .5, 0], [.5, .7, 0]], .05, .5, -1, both([Bx + [.7], A + [.5], A + [.5], Bx + [.5]], [1, 0, 1, 0])),
        # the same box three times in one class: IoU 1; the highest score survives, and of two equal scores the lower index
        'duplicate_boxes': ([A, A, A, Bx, Bx], [[.6, 0], [.9, 0], [.6, 0], [.4, 0], [.4, 0]], .05, .5, -1, both([A + [.9], Bx + [.4]], [0, 0])),
        # three disjoint boxes with one score, two wanted: rows 0 and 1
        'max_num_cuts_a_tie': ([A, Bx, Cx], [[.5, 0], [.5, 0], [.5, 0]], .05, .5, 2, both([A + [.5], Bx + [.5]], [0, 0])),
    }


def random_image(rows, C, box_cols, seed):
    """Overlapping boxes on a 200 x 200 canvas, scores with two decimals (many ties) -> (bboxes [rows, box_cols], scores [rows, C+1])."""
    rng = np.random.RandomState(seed)
    xy = rng.uniform(0, 160, (rows, box_cols // 4, 2))
    wh = rng.uniform(8, 60, (rows, box_cols // 4, 2))
    bboxes = np.concatenate([xy, xy + wh], 2).reshape(rows, box_cols).astype(F)
    scores = np.round(rng.rand(rows, C + 1), 2).astype(F)
    return bboxes, scores


def clustered_image(rows=5000, centres=40, seed=9):
    """One class, ``rows`` boxes jittered by a pixel or two around ``centres`` buildings: most are suppressed."""
    rng = np.random.RandomState(seed)
    cxy = rng.uniform(50, 950, (centres, 2))
    cwh = rng.uniform(30, 80, (centres, 2))
    k = rng.randint(0, centres, rows)
    xy = cxy[k] + rng.uniform(-2, 2, (rows, 2))
    wh = cwh[k] + rng.uniform(-2, 2, (rows, 2))
    bboxes = np.concatenate([xy, xy + wh], 1).astype(F)
    scores = np.stack([rng.uniform(0.06, 1, rows), np.zeros(rows)], 1).astype(F)
    return bboxes, scores
