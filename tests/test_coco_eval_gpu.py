"""GPU: COCO AP on the device (bonai_amd/csrc/coco_eval.hip, bonai_amd/coco_eval.py) against the numpy restatement of COCOeval
(tests/coco_eval_restatement.py, pinned by hand in tests/test_coco_eval_cpu.py).  Every comparison is EXACT: bit-equal float64
IoUs, equal match indices and bit words, bit-equal precision / recall arrays, equal summaries."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_eval_restatement as R  # noqa: E402
from test_validate_gpu import LOOSE, _synth_model, ds, files  # noqa: E402,F401  (the smallest model / dataset: its fixtures)

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 130)
NMAX = max(SIZES)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- IoU ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def box_case():
    """130 detections x 130 ground truths, the reference computed once: integer boxes on a grid of 10 (touching, nested, equal and
    disjoint pairs by construction) and boxes made from float32 corners as CocoDataset.xyxy2xywh makes them."""
    rng = np.random.RandomState(0)

    def boxes(n):
        grid = np.stack([rng.randint(0, 8, n) * 10, rng.randint(0, 8, n) * 10, rng.randint(1, 4, n) * 10, rng.randint(1, 4, n) * 10], 1)
        xyxy = rng.uniform(0, 90, (n, 4)).astype(np.float32)
        xyxy[:, 2:] = xyxy[:, :2] + rng.uniform(0.5, 40, (n, 2)).astype(np.float32)
        real = np.asarray([[r[0], r[1], r[2] - r[0], r[3] - r[1]] for r in xyxy.tolist()], np.float64)
        return np.where((np.arange(n) % 2 == 0)[:, None], grid.astype(np.float64), real)
    dt, gt = boxes(NMAX), boxes(NMAX)
    crowd = (rng.uniform(size=NMAX) < 0.2).astype(np.uint8)
    want = R.bb_iou(dt, gt, crowd)
    assert np.count_nonzero(want == 0) > 100 and np.count_nonzero(want == 1) >= 1 and np.count_nonzero((want > 0) & (want < 1)) > 100
    return dt, gt, crowd, want


@pytest.mark.parametrize('D', SIZES)
def test_box_iou_is_bit_equal(box_case, D):
    from bonai_amd import kernels as K
    dt, gt, crowd, want = box_case
    for G in SIZES:
        got = K.coco_box_iou(dt[:D], gt[:G], crowd[:G])
        assert got.dtype == torch.float64 and tuple(got.shape) == (D, G)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[:D, :G])), (D, G)


@pytest.fixture(scope='module')
def mask_case():
    """130 + 130 bitmaps of 64 x 48 pixels rasterised by kernels.poly2mask (rectangles and triangles, some outside each other,
    some empty after clipping), the reference computed once from the downloaded bitmaps."""
    from bonai_amd import kernels as K
    rng = np.random.RandomState(1)
    H, W = 48, 64

    def polys(n):
        out = []
        for i in range(n):
            x, y = rng.uniform(-4, W - 8), rng.uniform(-4, H - 8)
            w, h = rng.uniform(2, 30, 2)
            out.append([[x, y, x + w, y, x + w, y + h, x, y + h] if i % 3 else [x, y, x + w, y, x, y + h]])
        return out
    pm, gm = K.poly2mask(polys(NMAX), H, W), K.poly2mask(polys(NMAX), H, W)
    crowd = (rng.uniform(size=NMAX) < 0.2).astype(np.uint8)
    want = R.mask_iou(pm.cpu().numpy() != 0, gm.cpu().numpy() != 0, crowd)
    assert np.count_nonzero(want == 0) > 100 and np.count_nonzero(want > 0) > 100
    return pm, gm, crowd, want


@pytest.mark.parametrize('D', SIZES)
def test_mask_iou_is_bit_equal(mask_case, D):
    from bonai_amd import kernels as K
    pm, gm, crowd, want = mask_case
    H, W = pm.shape[1:]
    for G in SIZES:
        inter, area_p, area_g = K.mask_pair_counts(pm[:D].contiguous(), gm[:G].contiguous(), np.tile([0, 0, W, H], (D, 1)))
        got = K.coco_mask_iou(inter, area_p, area_g, crowd[:G])
        assert tuple(got.shape) == (D, G) and np.array_equal(_bits(got.cpu().numpy()), _bits(want[:D, :G])), (D, G)


# ---- matching -------------------------------------------------------------------------------------------------------------------

def _grid_boxes(rng, n):
    """Integer xywh boxes, coordinates up to 200, sides from a list whose products straddle 32^2 and 96^2."""
    side = np.asarray([8, 16, 24, 32, 40, 96, 104])
    w, h = side[rng.randint(0, side.size, n)], side[rng.randint(0, side.size, n)]
    x, y = rng.randint(0, 13, n) * 8, rng.randint(0, 13, n) * 8
    return np.stack([x, y, np.minimum(w, 200 - x), np.minimum(h, 200 - y)], 1).astype(np.float64)


@pytest.fixture(scope='module')
def segments():
    """One segment per (D, G) of {0, 1, 20, 21, 40} x {0, 1, 63, 64, 65, 130}.  Ground truths repeat (equal-IoU ties); detections
    are ground-truth boxes, their upper halves (IoU exactly 0.5) and other grid boxes."""
    rng = np.random.RandomState(2)
    out = []
    for D in (0, 1, 20, 21, 40):
        for G in SIZES:
            gt = _grid_boxes(rng, G)
            if G > 2:
                dup = rng.randint(0, G, G // 3)
                gt[dup] = gt[rng.randint(0, G, G // 3)]
            dt = _grid_boxes(rng, D)
            for d in range(D):
                if G and d % 4 != 3:
                    dt[d] = gt[rng.randint(0, G)]
                    if d % 4 == 1:
                        dt[d, 3] /= 2
            crowd = (rng.uniform(size=G) < 0.15).astype(np.uint8)
            out.append(SimpleNamespace(D=D, G=G, dt=dt, gt=gt, crowd=crowd, det_area=dt[:, 2] * dt[:, 3], gt_area=gt[:, 2] * gt[:, 3]))
    return out


def _pack(flags):
    """bool [T,D] per area range (list of A) -> uint64 words [D] with bit a*T + t."""
    T, D = flags[0].shape
    w = np.zeros(D, np.uint64)
    for a, f in enumerate(flags):
        for t in range(T):
            w |= f[t].astype(np.uint64) << np.uint64(a * T + t)
    return w


@pytest.mark.parametrize('T', (10, 1))
def test_matching_equals_evaluate_img(segments, T):
    from bonai_amd import kernels as K
    thrs = R.default_iou_thrs() if T == 10 else np.asarray([0.5])
    ious = [K.coco_box_iou(s.dt, s.gt, s.crowd) for s in segments]
    host = [x.cpu().numpy() for x in ious]
    for s, x in zip(segments, host):
        assert np.array_equal(_bits(x), _bits(R.bb_iou(s.dt, s.gt, s.crowd)))
    # the data holds what the rule is delicate about (checked on the host, before anything is compared)
    allv = np.concatenate([x.reshape(-1) for x in host])
    assert np.isin(allv, thrs).sum() >= 10                                                     # an IoU equal to a threshold
    assert sum(int(np.count_nonzero((x == x.max(1, keepdims=True)).sum(1)[x.max(1) >= 0.5] > 1)) for x in host if x.size) >= 10   # equal best IoUs
    assert sum(int(s.crowd.sum()) for s in segments) >= 10
    areas = np.concatenate([s.gt_area for s in segments] + [s.det_area for s in segments])
    assert all(np.count_nonzero(areas == v) for v in (32 ** 2, 96 ** 2)) and areas.min() < 32 ** 2 < 96 ** 2 < areas.max()
    assert any(s.D == 0 and s.G == 0 for s in segments)
    gt_match, bits, npig = K.coco_match(ious, [s.D for s in segments], [s.G for s in segments], np.concatenate([s.det_area for s in segments]),
                                        np.concatenate([s.gt_area for s in segments]), np.concatenate([s.crowd for s in segments]), thrs)
    gt_match, bits, npig = gt_match.cpu().numpy(), bits.cpu().numpy().view(np.uint64), npig.cpu().numpy()
    assert gt_match.shape == (sum(s.D for s in segments), 4, T) and npig.shape == (len(segments), 4)
    o, matched_total, tie_last = 0, 0, 0
    for j, (s, x) in enumerate(zip(segments, host)):
        evs = [R.evaluate_img(x, s.det_area, s.gt_area, s.crowd, rng, thrs) for rng in R.AREA_RNG]
        for a, ev in enumerate(evs):
            assert np.array_equal(gt_match[o:o + s.D, a, :].T, ev['dtm']), (s.D, s.G, a)
            assert npig[j, a] == ev['npig']
        assert np.array_equal(bits[o:o + s.D, 0], _pack([ev['dtm'] >= 0 for ev in evs])), (s.D, s.G)
        assert np.array_equal(bits[o:o + s.D, 1], _pack([ev['dt_ig'] for ev in evs])), (s.D, s.G)
        matched_total += int(np.count_nonzero(evs[0]['dtm'] >= 0))
        o += s.D
    assert matched_total > 100


def test_too_many_ground_truths_are_refused_before_any_launch():
    from bonai_amd import kernels as K
    from bonai_amd.lib import LoftHipError
    assert K.COCO_MAX_GT >= 4096
    with pytest.raises(LoftHipError, match=str(K.COCO_MAX_GT + 1)):
        K.coco_match(None, [3], [K.COCO_MAX_GT + 1], np.zeros(3), np.zeros(K.COCO_MAX_GT + 1), np.zeros(K.COCO_MAX_GT + 1), [0.5])
    with pytest.raises(LoftHipError, match='64'):
        K.coco_match(None, [0], [0], np.zeros(0), np.zeros(0), np.zeros(0), np.linspace(0.1, 0.9, 17))


# ---- accumulation ---------------------------------------------------------------------------------------------------------------

def _image_records(rng, total, T):
    """Per-image evaluateImg outputs with random flags, many equal scores, until ``total`` detections."""
    imgs, n = [], 0
    while n < total or not imgs:
        D = int(min(rng.randint(0, 24), total - n))
        scores = np.sort(rng.choice(np.asarray([0.125, 0.3, 0.3000001, 0.55, 0.9], np.float32), D))[::-1].copy()
        imgs.append(dict(scores=scores, dtm=[np.where(rng.uniform(size=(T, D)) < 0.5, 0, -1) for _ in range(4)],
                         dt_ig=[rng.uniform(size=(T, D)) < 0.2 for _ in range(4)], npig=[int(rng.randint(0, 6)), 0, int(rng.randint(0, 4)), 1]))
        n += D
        if total == 0:
            break
    return imgs


@pytest.mark.parametrize('T', (10, 1))
@pytest.mark.parametrize('total', (0, 1, 1023, 1024, 1025, 5000))
def test_accumulation_is_bit_equal(total, T):
    from bonai_amd import kernels as K
    rng = np.random.RandomState(total + T)
    imgs = _image_records(rng, total, T)
    assert sum(len(e['scores']) for e in imgs) == total
    max_dets, rec = (2, 5, 20), R.default_rec_thrs()
    scores = np.concatenate([e['scores'] for e in imgs]).astype(np.float32)
    rank = np.concatenate([np.arange(len(e['scores'])) for e in imgs]).astype(np.int32)
    words = np.stack([np.concatenate([_pack([f >= 0 for f in e['dtm']]) for e in imgs]),
                      np.concatenate([_pack(e['dt_ig']) for e in imgs])], 1).view(np.int64).reshape(-1, 2)
    npig = np.sum([e['npig'] for e in imgs], 0)
    assert npig[1] == 0 and npig[3] > 0                                       # an area range without ground truths stays -1
    p, r = K.coco_accumulate(scores, words, rank, npig, max_dets, rec, T)
    p, r = p.cpu().numpy(), r.cpu().numpy()
    assert p.shape == (T, 101, 4, 3) and r.shape == (T, 4, 3)
    for a in range(4):
        E = [dict(scores=e['scores'], dtm=e['dtm'][a], dt_ig=e['dt_ig'][a], npig=e['npig'][a]) for e in imgs]
        wp, wr = R.accumulate(E, max_dets, rec, T)
        assert np.array_equal(_bits(p[:, :, a, :]), _bits(wp)) and np.array_equal(_bits(r[:, a, :]), _bits(wr)), a
    assert np.all(p[:, :, 1, :] == -1) and np.all(r[:, 1, :] == -1)
    if total >= 1023:
        assert 0 < p[:, :, 0, :].max() <= 1                                   # (2 / (2 + 2^-52) rounds to 1)


# ---- end to end -----------------------------------------------------------------------------------------------------------------

def _rect(x, y, w, h):
    return [float(v) for v in (x, y, x + w, y, x + w, y + h, x, y + h)]


def _tiny_dataset():
    """Three 64 x 64 images (ids out of order), two categories, made-up annotations with their own ``area`` and a crowd."""
    rng = np.random.RandomState(3)
    infos = [dict(id=i, width=64, height=64) for i in (30, 10, 20)]
    anns, aid = [], 0
    for n, info in enumerate(infos):
        mine = []
        for k in range((7, 4, 9)[n]):
            x, y = rng.randint(0, 40, 2)
            w, h = rng.randint(6, 24, 2)
            aid += 1
            mine.append(dict(id=aid, image_id=info['id'], category_id=1 if (k % 3 or n == 1) else 2, iscrowd=int(k == 5),
                             bbox=[float(x), float(y), float(w), float(h)], area=float(w * h) - 0.5 * (k % 2),
                             segmentation=[_rect(x, y, w, h)] if k % 4 else [_rect(x, y, w, h / 2), _rect(x, y + h / 2, w / 2, h / 2)]))
        anns.append(mine)
    return SimpleNamespace(data_infos=infos, anns=anns, cat_ids=[1, 2])


def _tiny_detections(dsy, n):
    """Detections of image n: jittered ground-truth boxes and strays, float32 rows, equal scores among them; bitmaps rasterised
    from the jittered boxes cut at a corner (so the mask area differs from the box area)."""
    from bonai_amd import kernels as K
    rng = np.random.RandomState(10 + n)
    rows, labels, polys = [], [], []
    for a in dsy.anns[n] + [None] * (30 if n == 2 else 5):       # (image 2: more than 20 detections of one category -- the cut)
        if a is None:
            x, y, w, h = *rng.uniform(0, 40, 2), *rng.uniform(5, 20, 2)
            lab = int(rng.randint(0, 2)) if n == 0 else 0
        else:
            x, y, w, h = np.asarray(a['bbox']) + rng.uniform(-2, 2, 4) * (rng.uniform() < 0.7)
            lab = dsy.cat_ids.index(a['category_id'])
        rows.append([x, y, x + w, y + h, rng.choice([0.3, 0.5, 0.5, 0.8, 0.95])])
        labels.append(lab)
        polys.append([[x, y, x + w, y, x + w, y + h * 0.8, x + w * 0.8, y + h, x, y + h]])
    order = rng.permutation(len(rows))
    dets = np.asarray(rows, np.float32)[order]
    return dets, np.asarray(labels)[order], K.poly2mask([polys[i] for i in order], 64, 64)


def _restated(dsy, per_image, metric, max_dets, iou_thrs=None):
    """The restatement's CocoEval on the same data, in the result file's order (image, label, detection)."""
    from bonai_amd import kernels as K
    gts, dts = [], []
    for n, info in enumerate(dsy.data_infos):
        H, W = info['height'], info['width']
        gm = K.poly2mask([a['segmentation'] for a in dsy.anns[n]], H, W).cpu().numpy() != 0 if dsy.anns[n] else []
        gts += [dict(a, mask=gm[j]) for j, a in enumerate(dsy.anns[n])]
        dets, labels, masks = per_image[n]
        masks = masks.cpu().numpy() != 0
        for lab in range(len(dsy.cat_ids)):
            for i in np.where(np.asarray(labels) == lab)[0]:
                b = dets[i].tolist()
                dts.append(dict(image_id=info['id'], category_id=dsy.cat_ids[lab], score=float(dets[i][4]),
                                bbox=[b[0], b[1], b[2] - b[0], b[3] - b[1]], mask=masks[i]))
    e = R.CocoEval(gts, dts, [i['id'] for i in dsy.data_infos], dsy.cat_ids, metric, max_dets=max_dets, iou_thrs=iou_thrs)
    e.run()
    return e


@pytest.mark.parametrize('max_dets', ((100, 300, 1000), (2, 5, 20)))
def test_evaluator_equals_the_restatement_on_tiny_images(max_dets):
    from bonai_amd.coco_eval import CocoEvaluator, merge_records
    dsy = _tiny_dataset()
    per_image = [_tiny_detections(dsy, n) for n in range(3)]
    ev = CocoEvaluator(dsy, metrics=('bbox', 'segm'), proposal_nums=max_dets, batch_images=2)
    for n, (dets, labels, masks) in enumerate(per_image):
        ev.add_image(n, dets, labels, masks)
    got = ev.summarize()
    for metric in ('bbox', 'segm'):
        want = _restated(dsy, per_image, metric, max_dets)
        precision, recall = ev.accumulate(metric)
        assert np.array_equal(_bits(precision), _bits(want.precision)) and np.array_equal(_bits(recall), _bits(want.recall)), metric
        assert got['stats'][metric] == [float(v) for v in want.stats], metric
        for k, v in R.mmdet_keys(metric, want.stats).items():
            assert got[k] == v, k
        assert 0 < want.stats[1] < 1 and (want.stats[0] == -1) == (100 not in max_dets)
    assert set(got) == {f'{m}_{n}' for m in ('bbox', 'segm') for n in ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l', 'mAP_copypaste')} | {'stats'}
    # two shards (images i % 2), merged: the same records, the same summary
    shards = []
    for r in range(2):
        part = CocoEvaluator(dsy, metrics=('bbox', 'segm'), proposal_nums=max_dets)
        for n in range(r, 3, 2):
            part.add_image(n, *per_image[n])
        shards.append(part.records())
    merged, whole = merge_records(shards), ev.records()
    assert all(np.array_equal(merged[m][k], whole[m][k]) for m in merged for k in ('det', 'npig'))
    ev2 = CocoEvaluator(dsy, metrics=('bbox', 'segm'), proposal_nums=max_dets)
    ev2.load_records(merged)
    assert json.dumps(ev2.summarize()) == json.dumps(got)


def test_validator_reports_coco_ap_next_to_unchanged_bonai_metrics(ds):  # noqa: F811
    """The Validator with coco=...: the BONAI part equals a run without it, the training-state snapshot check passes (run()
    raises otherwise), and the coco dict equals the restatement fed with the same model's detections and bitmaps."""
    from bonai_amd.validate import Validator, val_line
    m = _synth_model().eval()
    base = Validator(m, ds, **LOOSE).run()
    v = Validator(m, ds, **LOOSE, coco=dict(metrics=['bbox', 'segm']))
    s = v.run()
    assert set(s) == {'roof', 'footprint', 'offset', 'coco'} and 'paste_min_score' not in m.roi_head.test_cfg
    assert json.dumps({k: s[k] for k in base}) == json.dumps(base)
    assert ', bbox_mAP: ' in val_line(1, 3, s) and ', segm_mAP_50: ' in val_line(1, 3, s) and 'mAP' not in val_line(1, 3, base)
    roi = m.roi_head
    roi.test_cfg['keep_device_masks'] = True
    roi.test_cfg['rle_masks'] = True
    per_image = []
    for i, data in ds.test_batches():
        with torch.no_grad():
            tup = m(return_loss=False, rescale=True, **data)
        assert sum(b.shape[0] for b in tup[0]) > 0
        per_image.append((np.array(roi.last_dets), np.array(roi.last_det_labels), roi.last_device_masks.clone()))
    print('detections per image:', [p[0].shape[0] for p in per_image])
    dsy = SimpleNamespace(data_infos=ds.data_infos, anns=ds.anns, cat_ids=ds.cat_ids)
    for metric in ('bbox', 'segm'):
        want = _restated(dsy, per_image, metric, (100, 300, 1000))
        assert s['coco']['stats'][metric] == [float(x) for x in want.stats], metric
        for k, x in R.mmdet_keys(metric, want.stats).items():
            assert s['coco'][k] == x, k
