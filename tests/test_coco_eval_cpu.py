"""CPU: COCO AP (bonai_amd/coco_eval.py).  pycocotools is not installed, so the numpy restatement the GPU tests compare against
(tests/coco_eval_restatement.py) is pinned here by answers derived by hand from COCOeval's rules; then the host surface:
cfg.evaluation.coco_ap, save_best='coco.*', the Epoch(val) line, and the merging of shards' records (alone and through a gloo
world of two)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_eval_restatement as R  # noqa: E402


def _gt(img, box, iscrowd=0, area=None, cat=1):
    return dict(image_id=img, category_id=cat, bbox=[float(v) for v in box], area=float(box[2] * box[3] if area is None else area),
                iscrowd=iscrowd)


def _dt(img, box, score, cat=1):
    return dict(image_id=img, category_id=cat, bbox=[float(v) for v in box], score=float(score))


def _run(gts, dts, img_ids=(1,), **kw):
    e = R.CocoEval(gts, dts, list(img_ids), [1], 'bbox', **kw)
    e.run()
    return e


FAR = [150, 150, 20, 20]


def test_tp_fp_tp_gives_the_101_point_average():
    """Two ground truths; detections TP (0.9), FP (0.8), TP (0.7): recall 0.5, 0.5, 1; precision 1, 1/2, 2/3, enveloped to
    1, 2/3, 2/3.  Recall thresholds <= 0.5 read precision 1, the others 2/3."""
    rec = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    assert np.array_equal(rec, R.default_rec_thrs()) and rec.size == 101
    n_first = int(np.count_nonzero(rec <= 0.5))                  # searchsorted(rc, thr, 'left') == 0  <=>  thr <= rc[0] = 0.5
    assert n_first == 51 and rec[50] == 0.5 and rec[51] > 0.5 and rec.size - n_first == 50
    e = _run([_gt(1, [10, 10, 20, 20]), _gt(1, [50, 50, 20, 20])],
             [_dt(1, [10, 10, 20, 20], 0.9), _dt(1, FAR, 0.8), _dt(1, [50, 50, 20, 20], 0.7)])
    want = (51 + 50 * (2 / 3)) / 101
    assert abs(e.stats[1] - want) <= 1e-12                       # AP at IoU 0.5
    assert abs(e.stats[0] - want) <= 1e-12 and abs(e.stats[3] - want) <= 1e-12        # IoU is 1: every threshold; area 400: small
    assert e.stats[4] == -1 and e.stats[5] == -1
    p = e.precision[0, :, 0, 0, 2]
    assert np.all(np.abs(p[:51] - 1) <= 1e-12) and np.all(np.abs(p[51:] - 2 / 3) <= 1e-12)
    assert e.recall[0, 0, 0, 2] == 1.0 and e.stats[8] == 1.0
    assert R.mmdet_keys('bbox', e.stats)['bbox_mAP'] == float(f'{want:.3f}') == 0.835


def test_perfect_detections_give_one_everywhere():
    boxes = [[10, 10, 20, 20], [50, 50, 50, 50], [0, 100, 100, 100]]          # small, medium, large
    e = _run([_gt(1, b) for b in boxes], [_dt(1, b, s) for b, s in zip(boxes, (0.9, 0.8, 0.7))])
    assert np.all(np.abs(e.stats - 1.0) <= 1e-12), e.stats
    keys = R.mmdet_keys('bbox', e.stats)
    assert all(keys[f'bbox_{n}'] == 1.0 for n in ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l'))
    assert keys['bbox_mAP_copypaste'] == '1.000 1.000 1.000 1.000 1.000 1.000'


def test_no_detections_give_zero_and_an_empty_range_minus_one():
    e = _run([_gt(1, [10, 10, 20, 20])], [])
    assert e.stats[0] == 0 and e.stats[1] == 0 and e.stats[3] == 0 and e.stats[6] == 0 and e.stats[8] == 0 and e.stats[9] == 0
    assert e.stats[4] == -1 and e.stats[5] == -1 and e.stats[10] == -1 and e.stats[11] == -1
    assert np.all(e.precision[:, :, 0, 0, :] == 0) and np.all(e.precision[:, :, 0, 2:, :] == -1)
    # entry 0 reads maxDets == 100 through the default argument: not in the list -> -1 (cocoapi's own quirk)
    e = _run([_gt(1, [10, 10, 20, 20])], [_dt(1, [10, 10, 20, 20], 0.9)], max_dets=(2, 5, 20))
    assert e.stats[0] == -1 and abs(e.stats[1] - 1) <= 1e-12 and e.stats[6] == 1.0


def test_a_crowd_absorbs_detections_as_neither_tp_nor_fp():
    """Three detections inside a crowd region score ABOVE the one true positive: counted as false positives they would push its
    precision to 1/4; matched to the crowd (IoU = intersection / detection area = 1, a crowd stays open) they are ignored."""
    gts = [_gt(1, [10, 10, 20, 20]), _gt(1, [100, 0, 80, 80], iscrowd=1)]
    inside = [[100, 0, 20, 20], [130, 10, 20, 20], [150, 50, 20, 20]]
    dts = [_dt(1, b, s) for b, s in zip(inside, (0.99, 0.98, 0.97))] + [_dt(1, [10, 10, 20, 20], 0.9)]
    e = _run(gts, dts)
    assert abs(e.stats[1] - 1) <= 1e-12 and abs(e.stats[0] - 1) <= 1e-12 and e.stats[8] == 1.0
    ev = e.eval_imgs[(1, 0, 1)]
    assert ev['npig'] == 1 and np.array_equal(ev['dtm'][0], [1, 1, 1, 0]) and np.array_equal(ev['dt_ig'][0], [True, True, True, False])
    for g in gts:
        g['iscrowd'] = 0
    plain = _run(gts, dts)
    assert plain.stats[1] < 0.2                                   # (the same boxes without the flag: three false positives first)


def test_an_iou_equal_to_the_threshold_matches():
    e = _run([_gt(1, [0, 0, 10, 10])], [_dt(1, [0, 0, 10, 5], 0.9)])
    assert R.bb_iou([[0, 0, 10, 5]], [[0, 0, 10, 10]], [0])[0, 0] == 0.5 == e.iou_thrs[0]
    ev = e.eval_imgs[(1, 0, 1)]
    assert ev['dtm'][0, 0] == 0 and np.all(ev['dtm'][1:, 0] == -1)
    assert abs(e.stats[1] - 1) <= 1e-12 and e.stats[2] == 0 and abs(e.stats[0] - 0.1) <= 1e-12


def test_an_area_of_exactly_32_squared_is_small_and_medium():
    e = _run([_gt(1, [0, 0, 32, 32])], [_dt(1, [0, 0, 32, 32], 0.9)])
    assert abs(e.stats[3] - 1) <= 1e-12 and abs(e.stats[4] - 1) <= 1e-12 and e.stats[5] == -1
    assert e.stats[9] == 1.0 and e.stats[10] == 1.0 and e.stats[11] == -1
    e = _run([_gt(1, [0, 0, 96, 96])], [_dt(1, [0, 0, 96, 96], 0.9)])
    assert e.stats[3] == -1 and abs(e.stats[4] - 1) <= 1e-12 and abs(e.stats[5] - 1) <= 1e-12


def test_of_two_equal_ious_the_later_ground_truth_is_taken():
    gts = [_gt(1, [0, 0, 10, 10]), _gt(1, [10, 0, 10, 10])]
    ious = R.bb_iou([[0, 0, 20, 10]], [g['bbox'] for g in gts], [0, 0])
    assert ious[0, 0] == ious[0, 1] == 0.5
    ev = R.evaluate_img(ious, [200.0], [100.0, 100.0], [0, 0], R.AREA_RNG[0], R.default_iou_thrs())
    assert ev['dtm'][0, 0] == 1 and ev['dtm'][1, 0] == -1
    # ... but a non-ignored match is not given up for an ignored ground truth of equal IoU that comes later in the visiting order
    ev = R.evaluate_img(ious, [200.0], [100.0, 100.0], [0, 1], R.AREA_RNG[0], R.default_iou_thrs())
    assert ev['dtm'][0, 0] == 0 and not ev['dt_ig'][0, 0]


def test_equal_scores_keep_input_order_and_image_id_order():
    """Images 7 and 3 (given in that order), one ground truth each, two detections of the same score each: image 3 (FP, TP),
    image 7 (TP, FP).  Sorted image ids and a stable sort give FP TP TP FP: precision 0, 1/2, 2/3, 1/2 -> envelope 2/3 up to
    recall 1.  Image 7 first, or TP before FP inside image 3, gives another number."""
    gts = [_gt(7, [10, 10, 20, 20]), _gt(3, [10, 10, 20, 20])]
    dts = [_dt(7, [10, 10, 20, 20], 0.5), _dt(7, FAR, 0.5), _dt(3, FAR, 0.5), _dt(3, [10, 10, 20, 20], 0.5)]
    e = _run(gts, dts, img_ids=(7, 3))
    assert e.img_ids == [3, 7]
    assert abs(e.stats[1] - 2 / 3) <= 1e-12 and np.all(np.abs(e.precision[0, :, 0, 0, 2] - 2 / 3) <= 1e-12)
    other = _run(gts, [dts[0], dts[1], dts[3], dts[2]], img_ids=(7, 3))         # TP before FP inside image 3: TP FP TP FP
    assert abs(other.stats[1] - (51 + 50 * (2 / 3)) / 101) <= 1e-12


def test_mask_iou_counts_pixels_with_the_crowd_rule():
    d = np.zeros((1, 8, 8), bool)
    d[0, :4, :4] = True
    g = np.zeros((2, 8, 8), bool)
    g[0, 2:6, 2:6] = True
    g[1, 6:, 6:] = True
    assert np.array_equal(R.mask_iou(d, g, [0, 0]), [[4 / 28, 0.0]])
    assert np.array_equal(R.mask_iou(d, g, [1, 1]), [[4 / 16, 0.0]])


# ---- the host surface -------------------------------------------------------------------------------------------------------

def test_parse_evaluation_with_and_without_coco_ap():
    from bonai_amd.validate import COCO_NOTICE, parse_evaluation
    said = []
    plain = parse_evaluation(dict(interval=1, metric=['bbox', 'segm']), log=said.append)
    assert plain == dict(interval=1, score_thr=0.4, min_area=500.0, iou_thr=0.5, save_best=None, num=None) and said == [COCO_NOTICE]
    assert parse_evaluation(dict(interval=1, metric=['bbox', 'segm'], coco_ap=False), log=said.append) == plain and len(said) == 2
    said.clear()
    ev = parse_evaluation(dict(interval=1, metric=['bbox', 'segm'], coco_ap=True, save_best='coco.segm_mAP'), log=said.append)
    assert said == [] and ev['coco'] == dict(metrics=['bbox', 'segm']) and ev['save_best'] == 'coco.segm_mAP'
    assert {k: v for k, v in ev.items() if k not in ('coco', 'save_best')} == {k: v for k, v in plain.items() if k != 'save_best'}
    assert parse_evaluation(dict(metric=['bonai', 'segm'], coco_ap=True), log=said.append)['coco'] == dict(metrics=['segm'])
    with pytest.raises(ValueError, match='coco.segm_mAP'):                       # only with coco_ap
        parse_evaluation(dict(metric=['bbox', 'segm'], save_best='coco.segm_mAP'), log=said.append)
    with pytest.raises(ValueError, match='coco.segm_mAP'):                       # ... and only for a metric that is computed
        parse_evaluation(dict(metric='bbox', coco_ap=True, save_best='coco.segm_mAP'), log=said.append)
    with pytest.raises(ValueError, match='footprint.mAP'):
        parse_evaluation(dict(metric=['bbox', 'segm'], coco_ap=True, save_best='footprint.mAP'), log=said.append)
    with pytest.raises(ValueError, match='coco_ap'):
        parse_evaluation(dict(metric='bonai', coco_ap=True), log=said.append)


def test_best_key_of_a_coco_number():
    from bonai_amd.validate import best_key, is_better
    assert best_key('coco.segm_mAP') == ('coco', 'segm_mAP', False) and best_key('coco.bbox_mAP_50') == ('coco', 'bbox_mAP_50', False)
    assert is_better('coco.segm_mAP', 0.3, 0.2) and not is_better('coco.segm_mAP', 0.2, 0.2) and is_better('coco.segm_mAP', 0.0, None)
    for bad in ('coco.segm_mAP_copypaste', 'coco.stats', 'coco.mAP', 'footprint.mAP'):
        with pytest.raises(ValueError, match=bad):
            best_key(bad)


def _summary():
    from bonai_amd import evaluation as E
    pair = lambda t, n, p: dict(gt_TP=list(range(t)), pred_TP=list(range(t)), gt_FN=list(range(n)), pred_FP=list(range(p)),
                                iou=np.zeros((t + p, t + n)))
    gt = np.asarray([[3.0, 4.0], [1.0, -2.0]], np.float32)
    return E.summarize([dict(roof=pair(2, 1, 0), footprint=pair(2, 0, 3), gt_offsets=gt, pred_offsets=gt + 1, num_pred=2, num_gt=3)])


def test_val_line_with_and_without_the_coco_dict():
    from bonai_amd.validate import val_line
    s = _summary()
    plain = val_line(3, 6, s)
    assert plain.startswith('Epoch(val) [3][6] roof_F1: ') and plain.endswith('pairs: 2') and 'mAP' not in plain
    s['coco'] = dict(bbox_mAP=0.412, bbox_mAP_50=0.7, bbox_mAP_copypaste='x', segm_mAP=0.375, segm_mAP_50=0.651, segm_mAP_75=0.2,
                     stats=dict(bbox=[0.0] * 12, segm=[0.0] * 12))
    assert val_line(3, 6, s) == plain + ', bbox_mAP: 0.4120, bbox_mAP_50: 0.7000, segm_mAP: 0.3750, segm_mAP_50: 0.6510'
    s['coco'] = dict(segm_mAP=0.375, segm_mAP_50=0.651)
    assert val_line(3, 6, s) == plain + ', segm_mAP: 0.3750, segm_mAP_50: 0.6510'


def _records(n_images=7, seed=0):
    """Hand-made per-image records in records()' layout: image ordinals NOT in the order the images are run."""
    rng = np.random.RandomState(seed)
    ordinal = rng.permutation(n_images)
    per_image = []
    for i in range(n_images):
        part = {}
        for metric in ('bbox', 'segm'):
            n = int(rng.randint(0, 6))
            det = np.zeros((n, 6), np.int64)
            det[:, 0], det[:, 2] = ordinal[i], np.arange(n)
            det[:, 3] = np.sort(rng.choice([0.25, 0.5, 0.75], n).astype(np.float32))[::-1].copy().view(np.int32)      # many equal scores
            det[:, 4:] = rng.randint(-2 ** 62, 2 ** 62, (n, 2))
            part[metric] = dict(det=det, npig=np.concatenate([[ordinal[i], 0], rng.randint(0, 9, 4)]).reshape(1, 6).astype(np.int64))
        per_image.append(part)
    return per_image


def _same_records(a, b):
    assert sorted(a) == sorted(b) == ['bbox', 'segm']
    for m in a:
        for k in ('det', 'npig'):
            assert a[m][k].dtype == np.int64 and np.array_equal(a[m][k], b[m][k]), (m, k)


def test_merge_records_of_a_two_way_split_equals_one_shard():
    from bonai_amd.coco_eval import merge_records
    imgs = _records()
    whole = merge_records(imgs)
    assert np.all(np.diff(whole['bbox']['det'][:, 0]) >= 0) and np.all(np.diff(whole['bbox']['npig'][:, 0]) > 0)
    d = whole['segm']['det']
    assert all(np.array_equal(d[d[:, 0] == o][:, 2], np.arange(np.count_nonzero(d[:, 0] == o))) for o in range(7))
    shards = [merge_records(imgs[r::2]) for r in range(2)]                     # the Validator's sharding: i % world == rank
    _same_records(merge_records(shards), whole)
    _same_records(merge_records(shards[::-1]), whole)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from bonai_amd.coco_eval import gather_records, merge_records
        imgs = _records()
        got = gather_records(merge_records(imgs[rank::world]), rank, world)      # shards of different lengths: padded
        _same_records(got, merge_records(imgs))
        q.put((rank, 'ok'))
    except Exception:  # noqa
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_gather_records_through_a_gloo_world_of_two():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(30)
    for rank, msg in res:
        assert msg == 'ok', f'rank {rank}: {msg}'


def test_stats_from_reads_the_max_dets_cocoapi_reads():
    """coco_eval.stats_from against the restatement's _summarizeDets on random precision / recall arrays (-1 planes included)."""
    from bonai_amd.coco_eval import stats_from
    rng = np.random.RandomState(1)
    for max_dets in ((100, 300, 1000), (2, 5, 20), (1, 10, 100)):
        e = R.CocoEval([], [], [1], [1, 2], 'bbox', max_dets=max_dets)
        e.precision = rng.uniform(0, 1, (10, 101, 2, 4, 3))
        e.recall = rng.uniform(0, 1, (10, 2, 4, 3))
        e.precision[:, :, 1, 2], e.recall[:, 1, 2] = -1, -1
        e.precision[:, :, :, 3], e.recall[:, :, 3] = -1, -1
        want = e.summarize()
        got = stats_from(e.precision, e.recall, e.iou_thrs, max_dets)
        assert got == [float(v) for v in want] and got[5] == -1 and got[11] == -1 and (got[0] == -1) == (100 not in max_dets)
