"""CPU: the host side of validation while training -- evaluation.merge_counts (dataset totals from additive partial sums, alone
and through a gloo world of 2), the parsing of cfg.evaluation, and the direction of save_best (bonai_amd/validate.py)."""
import itertools
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp


def _record(rng, n_pairs, tp=(2, 1), fn=(1, 0), fp=(0, 3), zero_gt=False):
    """A hand-made evaluate_image record: pairing lists of the given lengths and n_pairs paired offsets."""
    pair = lambda t, n, p: dict(gt_TP=list(range(t)), pred_TP=list(range(t)), gt_FN=list(range(n)), pred_FP=list(range(p)),
                                iou=np.zeros((t + p, t + n)))
    gt = rng.uniform(-30, 30, (n_pairs, 2)).astype(np.float32)
    if zero_gt and n_pairs:
        gt[0] = 0.0                                          # a zero vector: its cosine distance is nan (0 / 0), as in the reference
    return dict(roof=pair(tp[0], fn[0], fp[0]), footprint=pair(n_pairs, fn[1], fp[1]), gt_offsets=gt,
                pred_offsets=(gt + rng.normal(0, 3, gt.shape)).astype(np.float32), num_pred=tp[0] + fp[0], num_gt=tp[0] + fn[0])


def _records():
    rng = np.random.RandomState(0)
    return [_record(rng, 4), _record(rng, 0, tp=(0, 0), fn=(3, 3), fp=(2, 2)), _record(rng, 3, zero_gt=True), _record(rng, 7, fp=(5, 1)),
            _record(rng, 1, tp=(1, 1), fn=(0, 2)), _record(rng, 5, fn=(4, 4))]


def _assert_same(got, want, n_terms):
    """Integers and the maximum exactly; the means within the rounding of two different summation orders of n non-negative
    float64 terms: each order is off by at most (n - 1) u sum|x| and the division by half an ulp more, so the two means differ by
    at most 2 n u |mean| = n * 2^-52 * |mean| (EPE, AE and the cosine distance are all >= 0, so sum|x| = n * mean)."""
    for name in ('roof', 'footprint'):
        for k in ('TP', 'FN', 'FP'):
            assert got[name][k] == want[name][k] and isinstance(got[name][k], int)
        for k in ('F1_score', 'Precision', 'Recall'):
            assert got[name][k] == want[name][k] or (np.isnan(got[name][k]) and np.isnan(want[name][k]))
    assert got['offset']['pairs'] == want['offset']['pairs'] and got['offset']['max_EPE'] == want['offset']['max_EPE']
    for k in ('aEPE', 'aAE', 'cos_distance'):
        assert abs(got['offset'][k] - want['offset'][k]) <= n_terms * 2.0 ** -52 * abs(want['offset'][k]), k
    assert set(got) == set(want) and all(set(got[k]) == set(want[k]) for k in want)


def test_merge_counts_over_any_split_equals_summarize():
    from bonai_amd import evaluation as E
    recs = _records()
    want = E.summarize(recs)
    n = want['offset']['pairs']
    assert n == 20 and np.isfinite(want['offset']['cos_distance'])
    _assert_same(E.merge_counts(recs), want, n)                                           # records, one by one
    _assert_same(E.merge_counts([E.partial_counts(recs)]), want, n)                       # one shard
    for cuts in itertools.chain.from_iterable(itertools.combinations(range(1, len(recs)), k) for k in (1, 2, 3)):
        b = [0, *cuts, len(recs)]
        shards = [recs[i:j] for i, j in zip(b[:-1], b[1:])]
        _assert_same(E.merge_counts([E.partial_counts(s) for s in shards]), want, n)
    _assert_same(E.merge_counts([E.partial_counts(recs[0::2]), *recs[1::2]]), want, n)    # interleaved, partials and records mixed
    # nothing paired anywhere: the nan layout of summarize
    empty = E.merge_counts([recs[1]])
    ref = E.summarize([recs[1]])
    assert empty['offset']['pairs'] == 0 and all(np.isnan(empty['offset'][k]) and np.isnan(ref['offset'][k])
                                                   for k in ('aEPE', 'aAE', 'max_EPE'))
    assert all(empty[n][k] == ref[n][k] for n in ('roof', 'footprint') for k in ('TP', 'FN', 'FP'))


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
        from bonai_amd import evaluation as E
        from bonai_amd.validate import reduce_counts
        recs = _records()
        mine = [r for i, r in enumerate(recs) if i % world == rank]               # the Validator's sharding
        got = E.merge_counts([reduce_counts(E.partial_counts(mine), rank, world)])
        want = E.summarize(recs)
        _assert_same(got, want, want['offset']['pairs'])
        q.put((rank, 'ok'))
    except Exception:  # noqa
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_merge_counts_through_a_gloo_world_of_two():
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


def test_parse_evaluation_keys_notice_and_unknown_key():
    from bonai_amd.validate import COCO_NOTICE, parse_evaluation
    said = []
    ev = parse_evaluation(dict(interval=2, metric='bonai', score_thr=0.3, min_area=100, iou_thr=0.6, save_best='offset.aEPE', num=5),
                          log=said.append)
    assert ev == dict(interval=2, score_thr=0.3, min_area=100.0, iou_thr=0.6, save_best='offset.aEPE', num=5) and said == []
    ev = parse_evaluation(dict(interval=1, metric=['bbox', 'segm']), log=said.append)      # the reference's configs
    assert ev == dict(interval=1, score_thr=0.4, min_area=500.0, iou_thr=0.5, save_best=None, num=None)
    assert said == [COCO_NOTICE] and 'pycocotools' in COCO_NOTICE and 'bonai_evaluation.py' in COCO_NOTICE
    assert parse_evaluation(None, log=said.append)['interval'] == 1 and len(said) == 1
    with pytest.raises(KeyError, match='gpu_collect'):
        parse_evaluation(dict(interval=1, gpu_collect=True), log=said.append)
    with pytest.raises(ValueError, match='proposal'):
        parse_evaluation(dict(metric='proposal'), log=said.append)
    with pytest.raises(ValueError, match='footprint.mAP'):
        parse_evaluation(dict(save_best='footprint.mAP'), log=said.append)


def test_save_best_direction():
    from bonai_amd.validate import best_key, is_better
    assert best_key('footprint.F1_score') == ('footprint', 'F1_score', False)
    assert best_key('offset.aEPE')[2] and best_key('offset.aAE')[2] and not best_key('roof.Recall')[2]
    assert is_better('footprint.F1_score', 0.1, None) and is_better('footprint.F1_score', 0.6, 0.5)
    assert not is_better('footprint.F1_score', 0.4, 0.5) and not is_better('footprint.F1_score', 0.5, 0.5)
    assert is_better('offset.aEPE', 4.0, 5.0) and not is_better('offset.aEPE', 6.0, 5.0) and is_better('offset.aAE', 0.1, 0.2)
    assert not is_better('offset.aEPE', float('nan'), None) and not is_better('footprint.F1_score', float('nan'), 0.2)


def test_val_line_names_the_metrics():
    from bonai_amd import evaluation as E
    from bonai_amd.validate import val_line
    line = val_line(3, 6, E.summarize(_records()))
    assert line.startswith('Epoch(val) [3][6] roof_F1: ')
    for word in ('footprint_F1: ', 'roof_precision: ', 'footprint_recall: ', 'aEPE: ', 'aAE: ', 'pairs: 20'):
        assert word in line
