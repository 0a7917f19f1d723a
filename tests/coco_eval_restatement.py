"""A numpy / plain-Python restatement of COCOeval for the tests of bonai_amd/coco_eval.py: computeIoU (bbIou / rleIou of
common/maskApi.c), evaluateImg, accumulate and _summarizeDets of the published cocoapi source
(PythonAPI/pycocotools/cocoeval.py), in float64, loop for loop.  It shares no code with bonai_amd/coco_eval.py or the kernels.
pycocotools is not installed here: this file has not been run against it, and tests/test_coco_eval_cpu.py pins it with
hand-derived answers instead.

Differences in form only: the matched ground truth is kept as an INDEX (-1: none) instead of an annotation id, so "matched" is
`index >= 0` where cocoapi tests `dtm != 0` (the same whenever no annotation id is 0), and masks are boolean arrays instead of
RLE strings (rleIou counts the same pixels)."""
import numpy as np

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def default_iou_thrs():
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def default_rec_thrs():
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def bb_iou(dt, gt, iscrowd):
    """maskApi.c bbIou: dt [D,4], gt [G,4] xywh -> [D,G] (Python floats are C doubles)."""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 4).tolist(), np.asarray(gt, np.float64).reshape(-1, 4).tolist()
    o = np.zeros((len(dt), len(gt)), np.float64)
    for g, G in enumerate(gt):
        ga = G[2] * G[3]
        crowd = bool(iscrowd[g])
        for d, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


def mask_iou(dm, gm, iscrowd):
    """maskApi.c rleIou on bitmaps: dm [D,H,W], gm [G,H,W] bool -> [D,G].  (Its bounding-box pre-test only skips pairs whose
    intersection is empty, and those give 0 / 1 = 0 anyway.)"""
    dm, gm = np.asarray(dm).astype(bool), np.asarray(gm).astype(bool)
    o = np.zeros((dm.shape[0], gm.shape[0]), np.float64)
    for g in range(gm.shape[0]):
        for d in range(dm.shape[0]):
            i = int(np.count_nonzero(dm[d] & gm[g]))
            if i == 0:
                u = 1
            elif iscrowd[g]:
                u = int(np.count_nonzero(dm[d]))
            else:
                u = int(np.count_nonzero(dm[d] | gm[g]))
            o[d, g] = float(i) / float(u)
    return o


def evaluate_img(ious, det_area, gt_area, gt_crowd, a_rng, iou_thrs):
    """cocoeval.py evaluateImg for one (image, category, area range).  ious [D,G]: detections ALREADY in stable descending score
    order and cut to maxDet, ground truths in input order.  -> dict(dtm int [T,D]: index (input order) of the matched ground
    truth or -1; dt_ig bool [T,D]; gt_ig bool [G] in input order; npig)."""
    ious = np.asarray(ious, np.float64)
    D, G = len(det_area), len(gt_area)
    ious = ious.reshape(D, G)
    T = len(iou_thrs)
    ignore = [1 if (gt_crowd[g] or gt_area[g] < a_rng[0] or gt_area[g] > a_rng[1]) else 0 for g in range(G)]
    gtind = np.argsort(ignore, kind='mergesort')
    gt_ig = np.array([ignore[g] for g in gtind], dtype=np.int64)
    iscrowd = [int(gt_crowd[g]) for g in gtind]
    ious_s = ious[:, gtind] if G else ious
    gtm = np.zeros((T, G), np.int64)
    dtm = -np.ones((T, D), np.int64)
    dt_ig = np.zeros((T, D), bool)
    if G and D:
        for tind, t in enumerate(iou_thrs):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious_s[dind, gind] < iou:
                        continue
                    iou = ious_s[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = gtind[m]
                gtm[tind, m] = 1
    a = np.array([det_area[d] < a_rng[0] or det_area[d] > a_rng[1] for d in range(D)], dtype=bool).reshape((1, D))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm < 0, np.repeat(a, T, 0)))
    return dict(dtm=dtm, dt_ig=dt_ig, gt_ig=np.array(ignore, dtype=bool), npig=int(np.count_nonzero(gt_ig == 0)))


def accumulate(E, max_dets, rec_thrs, T):
    """cocoeval.py accumulate for one (category, area range).  E: per image, in image-id order, dict(scores [D] in the order of
    evaluate_img's detections, dtm [T,D], dt_ig [T,D], npig).  -> (precision [T,R,M], recall [T,M])."""
    R, M = len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, M))
    recall = -np.ones((T, M))
    for m, max_det in enumerate(max_dets):
        if len(E) == 0:
            continue
        scores = np.concatenate([np.asarray(e['scores'], np.float64)[0:max_det] for e in E])
        inds = np.argsort(-scores, kind='mergesort')
        dtm = np.concatenate([e['dtm'][:, 0:max_det] for e in E], axis=1)[:, inds]
        dt_ig = np.concatenate([e['dt_ig'][:, 0:max_det] for e in E], axis=1)[:, inds]
        npig = sum(e['npig'] for e in E)
        if npig == 0:
            continue
        tps = np.logical_and(dtm >= 0, np.logical_not(dt_ig))
        fps = np.logical_and(np.logical_not(dtm >= 0), np.logical_not(dt_ig))
        tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
        fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
        for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
            tp, fp = np.array(tp), np.array(fp)
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            q = np.zeros((R,))
            recall[t, m] = rc[-1] if nd else 0
            pr = pr.tolist()
            q = q.tolist()
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            inds_r = np.searchsorted(rc, rec_thrs, side='left')
            try:
                for ri, pi in enumerate(inds_r):
                    q[ri] = pr[pi]
            except IndexError:
                pass
            precision[t, :, m] = np.array(q)
    return precision, recall


class CocoEval:
    """COCOeval(cocoGt, cocoDt, iouType) with params.imgIds / catIds / maxDets / iouThrs set as mmdet's CocoDataset.evaluate sets
    them.  gts: dicts(image_id, category_id, bbox xywh, area, iscrowd[, mask bool [H,W]]); dts: dicts(image_id, category_id, score,
    bbox xywh | mask bool [H,W]) in result-file order; a detection's area is w*h (bbox) or its pixel count (segm), as loadRes
    sets it."""

    def __init__(self, gts, dts, img_ids, cat_ids, iou_type='bbox', max_dets=(100, 300, 1000), iou_thrs=None):
        self.iou_type = iou_type
        self.img_ids = list(np.unique(img_ids))
        self.cat_ids = list(np.unique(cat_ids))
        self.max_dets = list(max_dets)
        self.iou_thrs = default_iou_thrs() if iou_thrs is None else np.asarray(iou_thrs, np.float64)
        self.rec_thrs = default_rec_thrs()
        self.gts, self.dts = {}, {}
        for g in gts:
            if g['image_id'] in self.img_ids and g['category_id'] in self.cat_ids:
                self.gts.setdefault((g['image_id'], g['category_id']), []).append(g)
        for d in dts:
            if d['image_id'] in self.img_ids and d['category_id'] in self.cat_ids:
                d = dict(d)
                d['area'] = float(d['bbox'][2] * d['bbox'][3]) if iou_type == 'bbox' else float(np.count_nonzero(d['mask']))
                self.dts.setdefault((d['image_id'], d['category_id']), []).append(d)

    def _sorted_dets(self, key):
        dt = self.dts.get(key, [])
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        return [dt[i] for i in inds[0:self.max_dets[-1]]]

    def compute_iou(self, key):
        gt, dt = self.gts.get(key, []), self._sorted_dets(key)
        if len(gt) == 0 and len(dt) == 0:
            return []
        iscrowd = [int(o['iscrowd']) for o in gt]
        if self.iou_type == 'segm':
            shape = (dt + gt)[0]['mask'].shape
            return mask_iou(np.array([d['mask'] for d in dt], bool).reshape((-1,) + shape),
                            np.array([g['mask'] for g in gt], bool).reshape((-1,) + shape), iscrowd)
        return bb_iou([d['bbox'] for d in dt], [g['bbox'] for g in gt], iscrowd)

    def evaluate(self):
        self.eval_imgs = {}
        for k in self.cat_ids:
            for i in self.img_ids:
                gt, dt = self.gts.get((i, k), []), self._sorted_dets((i, k))
                if len(gt) == 0 and len(dt) == 0:
                    continue
                ious = np.asarray(self.compute_iou((i, k)), np.float64).reshape(len(dt), len(gt))
                for a, rng in enumerate(AREA_RNG):
                    e = evaluate_img(ious, [d['area'] for d in dt], [g['area'] for g in gt], [g['iscrowd'] for g in gt], rng,
                                     self.iou_thrs)
                    e['scores'] = [d['score'] for d in dt]
                    self.eval_imgs[(k, a, i)] = e
        return self

    def accumulate(self):
        T, R, K, A, M = len(self.iou_thrs), len(self.rec_thrs), len(self.cat_ids), len(AREA_RNG), len(self.max_dets)
        self.precision = -np.ones((T, R, K, A, M))
        self.recall = -np.ones((T, K, A, M))
        for ki, k in enumerate(self.cat_ids):
            for a in range(A):
                E = [self.eval_imgs[(k, a, i)] for i in self.img_ids if (k, a, i) in self.eval_imgs]
                p, r = accumulate(E, self.max_dets, self.rec_thrs, T)
                self.precision[:, :, ki, a, :] = p
                self.recall[:, ki, a, :] = r
        return self

    def _summarize(self, ap=1, iou_thr=None, area_rng='all', max_dets=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area_rng]
        mind = [i for i, m in enumerate(self.max_dets) if m == max_dets]
        s = self.precision if ap == 1 else self.recall
        if iou_thr is not None:
            t = np.where(iou_thr == self.iou_thrs)[0]
            s = s[t]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    def summarize(self):
        md = self.max_dets
        st = np.zeros((12,))
        st[0] = self._summarize(1)
        st[1] = self._summarize(1, iou_thr=.5, max_dets=md[2])
        st[2] = self._summarize(1, iou_thr=.75, max_dets=md[2])
        st[3] = self._summarize(1, area_rng='small', max_dets=md[2])
        st[4] = self._summarize(1, area_rng='medium', max_dets=md[2])
        st[5] = self._summarize(1, area_rng='large', max_dets=md[2])
        st[6] = self._summarize(0, max_dets=md[0])
        st[7] = self._summarize(0, max_dets=md[1])
        st[8] = self._summarize(0, max_dets=md[2])
        st[9] = self._summarize(0, area_rng='small', max_dets=md[2])
        st[10] = self._summarize(0, area_rng='medium', max_dets=md[2])
        st[11] = self._summarize(0, area_rng='large', max_dets=md[2])
        self.stats = st
        return st

    def run(self):
        self.evaluate().accumulate()
        return self.summarize()


def mmdet_keys(metric, stats):
    """The dictionary entries CocoDataset.evaluate (mmdet/datasets/coco.py:528-542) makes of ``stats`` for one metric."""
    names = ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']
    out = {f'{metric}_{n}': float(f'{stats[i]:.3f}') for i, n in enumerate(names)}
    ap = stats[:6]
    out[f'{metric}_mAP_copypaste'] = f'{ap[0]:.3f} {ap[1]:.3f} {ap[2]:.3f} {ap[3]:.3f} {ap[4]:.3f} {ap[5]:.3f}'
    return out
