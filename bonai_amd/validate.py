"""The validation pass as a library: the loop tools/test.py runs over a dataset, and a Validator that runs it between two
training steps (the reference's EvalHook, apis/train.py:113-126, with the BONAI metrics of tools/bonai/bonai_evaluation.py in
place of COCO AP).

What a pass between two ``Trainer.train_step`` calls has to respect, and how:
  * current weights: the fused optimizers write the arena through raw pointers, so no ``Tensor._version`` moves.  The
    version-keyed operand caches (nn._pack_cache_*) are only ever filled for parameters with requires_grad=False, which are
    not in the arena and are never written; every trainable layer folds and packs its operands anew at each forward outside a
    trainer step (nn.PREPACK is None there).  Nothing has to be invalidated (tests/test_validate_gpu.py pins it).
  * training state: the pass draws no random number (the RandomSampler counter is checked), does not touch the trainer, and
    leaves the process-global hand-over tables (nn.PREPACK, kernels.WEIGHT_PLANES, nn.JOIN, nn.PAIR_G) as it found them.
    Between two steps they are all unset / empty: only nn.installed() sets them, inside the scopes of Trainer.train_step, which
    put back what they found however the step ends (a raise included) and clear nn.PAIR_G on the way out.
  * it runs uncaptured; tools/train.py refuses --graph together with validation.
"""
import numpy as np
import torch

from . import evaluation as E


def paste_windows(boxes):
    """Half-open pixel windows that contain every pixel kernels.mask_paste sets for ``boxes`` [n,>=4] (it paints inside
    [floor(x1) - 1, ceil(x2) + 1)): what evaluation.evaluate_image hands kernels.mask_pair_counts."""
    b = np.asarray(boxes, np.float32)
    b = b.reshape(-1, b.shape[-1] if b.ndim == 2 else 5)
    return np.stack([np.floor(b[:, 0]) - 2, np.floor(b[:, 1]) - 2, np.ceil(b[:, 2]) + 2, np.ceil(b[:, 3]) + 2], 1)


def run_dataset(model, ds, evaluate=False, eval_kw=None, log=print, indices=None, coco=None):
    """-> (results as single_gpu_test returns them, per-image evaluation records or None).  ``indices``: the images to run
    (default: all of them, in order).  ``coco``: a coco_eval.CocoEvaluator that is fed every image's detections and pasted
    bitmaps (needs evaluate=True)."""
    roi = model.roi_head
    # rle_masks='fused' (tools/test.py --fused-rle / --footprints): strings from the logits, no bitmaps -- nothing to evaluate on
    fused = roi.test_cfg.get('rle_masks', False) == 'fused'
    if fused and evaluate:
        raise ValueError("run_dataset(evaluate=True) pairs buildings on the pasted bitmaps, rle_masks='fused' builds none")
    if not fused:
        roi.test_cfg['keep_device_masks'] = True
        # simple_test encodes the pasted device bitmaps as RLE itself (one pass): without this it also copied every detection's
        # full-image bool mask to the host (up to 100 x 1 MiB per tile) for a result this loop then threw away
        roi.test_cfg['rle_masks'] = True
    results, records = [], ([] if evaluate else None)
    for i, data in (ds.test_batches() if indices is None else ds.test_batches(indices=[int(i) for i in indices])):
        with torch.no_grad():
            res = tuple(model(return_loss=False, rescale=True, **data))      # a 4-tuple with test_cfg.rcnn.footprint_rle
        bbox_res, segm, off_res = res[:3]
        n_det = sum(b.shape[0] for b in bbox_res)
        pasted = roi.last_device_masks if n_det and not fused else None
        results.append(res)
        if evaluate:
            h, w = data['img_metas'][0][0]['ori_shape'][:2]
            pm = pasted if pasted is not None else torch.zeros(0, h, w, dtype=torch.uint8, device=data['img'][0].device)
            boxes = roi.last_dets if pasted is not None else np.zeros((0, 5), np.float32)
            offs = np.asarray(off_res, np.float32).reshape(-1, 2) if pasted is not None else np.zeros((0, 2), np.float32)
            records.append(E.evaluate_image(pm, boxes, offs, ds.get_ann_info(i), **(eval_kw or {})))
            if coco is not None:
                if n_det and pasted is None:
                    raise ValueError('COCO AP is fed from the pasted device bitmaps (roi.last_device_masks); this model pasted none')
                labels = roi.last_det_labels if pasted is not None else np.zeros(0, np.int64)
                coco.add_image(i, boxes, labels, pm, mask_windows=paste_windows(boxes))
        if (i + 1) % 50 == 0 or i + 1 == len(ds):
            log(f'[{i + 1}/{len(ds)}]')
    return results, records


def _globals_snapshot():
    from . import kernels as K
    from . import nn as F2
    return (F2.PREPACK, K.WEIGHT_PLANES, F2.JOIN, sorted(F2.PAIR_G), int(K._SAMPLE_CALLS[0]))


def reduce_counts(part, rank, world, device=None):
    """evaluation.partial_counts of this rank -> the totals over all ranks, with ONE SUM all-reduce of a small float64 vector.
    The maximum rides in it: every rank writes its own into its slot of a world-sized tail of zeros, so the sum hands every rank
    all the maxima (x + 0 is exact).  Counts are far below 2^53: exact in float64.  ``device``: where the vector lives for a
    backend that reduces device memory (nccl)."""
    import torch.distributed as dist
    keys = [k for k in E._COUNT_KEYS if k != 'max_EPE']
    vec = torch.zeros(len(keys) + world, dtype=torch.float64)
    for j, k in enumerate(keys):
        vec[j] = float(part[k])
    vec[len(keys) + rank] = part['max_EPE']
    if dist.get_backend() == 'nccl':
        vec = vec.to(device)
    dist.all_reduce(vec)
    vec = vec.cpu()
    out = {k: (float(vec[j]) if k.startswith('sum_') else int(round(float(vec[j])))) for j, k in enumerate(keys)}
    out['max_EPE'] = float(vec[len(keys):].max())
    return out


class Validator:
    """Validation of ``model`` on ``dataset`` (a BonaiDataset in test mode) with the BONAI metrics.

        Validator(model, dataset, score_thr=0.4, min_area=500, iou_thr=0.5, rank=0, world=1).run() -> summarize's layout

    Rank r of ``world`` takes the images i % world == r; the shards' additive partial sums (evaluation.partial_counts) are
    combined with ONE all-reduce and turned into the totals by evaluation.merge_counts, so every rank returns the same summary.
    The model runs in eval() under no_grad and is put back into the mode it was in.  The RoI head pastes only detections the
    metric keeps (test_cfg.rcnn['paste_min_score'] = score_thr for the duration of the pass).

    ``coco``: dict(metrics=['bbox', 'segm'][, proposal_nums, iou_thrs]) (parse_evaluation's ``coco`` entry) adds COCO AP
    (bonai_amd/coco_eval.py) as the summary's ``coco`` dict.  AP needs every detection up to proposal_nums[-1] and, for 'segm',
    its bitmap, so paste_min_score is then NOT set; the BONAI metrics filter by score on the host anyway and are unchanged.  With
    world > 1 the shards' compact records are all-gathered and every rank accumulates the same totals."""

    def __init__(self, model, dataset, score_thr=0.4, min_area=500, iou_thr=0.5, rank=0, world=1, num=None, coco=None):
        self.model, self.dataset = model, dataset
        self.coco = dict(coco) if coco else None
        self.eval_kw = dict(score_thr=score_thr, min_area=min_area, iou_thr=iou_thr)
        self.rank, self.world = int(rank), int(world)
        self.num = len(dataset) if num is None else min(int(num), len(dataset))
        self.results = self.records = None   # the last pass's result tuples and per-image records of this rank

    def indices(self):
        return [i for i in range(self.num) if i % self.world == self.rank]

    def run(self, log=lambda *_: None):
        model, roi = self.model, self.model.roi_head
        was_training = model.training
        before = _globals_snapshot()
        cfg = roi.test_cfg
        missing = object()
        saved = {k: cfg.get(k, missing) for k in ('paste_min_score', 'keep_device_masks', 'rle_masks')}
        evaluator = None
        if self.coco is not None:
            from .coco_eval import CocoEvaluator
            evaluator = CocoEvaluator(self.dataset, device=next(model.parameters()).device, **self.coco)
            cfg.pop('paste_min_score', None)
        else:
            cfg['paste_min_score'] = self.eval_kw['score_thr']
        model.eval()
        try:
            with torch.no_grad():
                self.results, self.records = run_dataset(model, self.dataset, evaluate=True, eval_kw=self.eval_kw, log=log,
                                              indices=self.indices(), coco=evaluator)
                if evaluator is not None:
                    evaluator.flush()
        finally:
            for k, v in saved.items():
                if v is missing:
                    cfg.pop(k, None)
                else:
                    cfg[k] = v
            roi.last_device_masks = None                    # (up to hundreds of MiB of bitmaps: not kept into the next step)
            if was_training:
                model.train()
        after = _globals_snapshot()
        if after[0] is not before[0] or after[1] is not before[1] or after[2] is not before[2] or after[3] != before[3] \
                or after[4] != before[4]:
            raise RuntimeError('the validation pass changed training state (nn.PREPACK / kernels.WEIGHT_PLANES / nn.JOIN / '
                               f'nn.PAIR_G / sampler draws): {before} -> {after}')
        part = E.partial_counts(self.records)
        if self.world > 1:
            part = reduce_counts(part, self.rank, self.world, next(self.model.parameters()).device)
        summary = E.merge_counts([part])
        if evaluator is not None:
            if self.world > 1:
                from .coco_eval import gather_records
                evaluator.load_records(gather_records(evaluator.records(), self.rank, self.world, next(self.model.parameters()).device))
            summary['coco'] = evaluator.summarize()
        return summary


# ---- the config surface of tools/train.py ------------------------------------------------------------------------------------

EVAL_KEYS = ('interval', 'metric', 'score_thr', 'min_area', 'iou_thr', 'save_best', 'num', 'coco_ap')
COCO_NOTICE = ("evaluation.metric=['bbox', 'segm'] asks for COCO AP, which needs pycocotools; it is not available here: the BONAI "
               'metrics of tools/bonai/bonai_evaluation.py (roof / footprint F1, offset aEPE / aAE) are reported instead')


def parse_evaluation(evaluation, log=print):
    """cfg.evaluation -> dict(interval, score_thr, min_area, iou_thr, save_best, num).  ``metric`` may be 'bonai' or the
    reference's COCO names ('bbox' / 'segm', alone or in a list): those print COCO_NOTICE once and give the BONAI metrics.
    An unknown key, an unknown metric or a save_best that names no number of the summary raises, naming it.
    ``coco_ap=True`` (opt-in): 'bbox' / 'segm' are computed (bonai_amd/coco_eval.py) next to the BONAI metrics, the notice is not
    printed, the result gains ``coco=dict(metrics=[...])`` for the Validator and save_best may name a 'coco.*' number."""
    ev = dict(evaluation or {})
    unknown = sorted(k for k in ev if k not in EVAL_KEYS)
    if unknown:
        raise KeyError(f'cfg.evaluation: unknown key {unknown[0]!r} (accepted: {", ".join(EVAL_KEYS)})')
    metric = ev.get('metric', 'bonai')
    names = [metric] if isinstance(metric, str) else list(metric)
    bad = [m for m in names if m not in ('bonai', 'bbox', 'segm')]
    if bad or not names:
        raise ValueError(f"cfg.evaluation.metric: {metric!r} is not 'bonai' or the reference's ['bbox', 'segm']")
    coco = [m for m in names if m != 'bonai'] if ev.get('coco_ap') else None
    if ev.get('coco_ap') and not coco:
        raise ValueError(f"cfg.evaluation.coco_ap: metric {metric!r} names neither 'bbox' nor 'segm'")
    if coco is None and any(m != 'bonai' for m in names):
        log(COCO_NOTICE)
    out = dict(interval=int(ev.get('interval', 1)), score_thr=float(ev.get('score_thr', 0.4)), min_area=float(ev.get('min_area', 500)),
               iou_thr=float(ev.get('iou_thr', 0.5)), save_best=ev.get('save_best'), num=ev.get('num'))
    if out['interval'] < 1:
        raise ValueError(f"cfg.evaluation.interval must be a positive number of epochs, got {ev.get('interval')!r}")
    if coco is not None:
        out['coco'] = dict(metrics=coco)
    if out['save_best'] is not None:
        best_key(out['save_best'], coco=coco)
    return out


_SUMMARY_KEYS = {'roof': ('F1_score', 'Precision', 'Recall', 'TP', 'FN', 'FP'), 'footprint': ('F1_score', 'Precision', 'Recall', 'TP', 'FN', 'FP'),
                 'offset': ('aEPE', 'aAE', 'cos_distance', 'max_EPE', 'pairs')}


_COCO_KEYS = tuple(f'{m}_{n}' for m in ('bbox', 'segm') for n in ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l'))


def best_key(save_best, coco=('bbox', 'segm')):
    """'name.key' of the summary -> (name, key, lower_is_better).  Lower is better for offset.aEPE and offset.aAE only.
    'coco.<metric>_mAP...' (higher is better) names a number of the summary's ``coco`` dict: ``coco`` = the metrics it will
    hold (parse_evaluation passes None without coco_ap, and the name is then refused like any other unknown one)."""
    name, _, key = str(save_best).partition('.')
    if name == 'coco' and key in _COCO_KEYS and key.split('_')[0] in (coco or ()):
        return name, key, False
    if key not in _SUMMARY_KEYS.get(name, ()):
        raise ValueError(f'cfg.evaluation.save_best: {save_best!r} is not a name.key of the summary '
                         f'({", ".join(n + "." + k for n, ks in _SUMMARY_KEYS.items() for k in ks)})')
    return name, key, (name, key) in (('offset', 'aEPE'), ('offset', 'aAE'))


def is_better(save_best, value, best):
    """Does ``value`` beat the best so far (None: nothing yet)?  nan never does."""
    lower = best_key(save_best)[2]
    if value is None or value != value:
        return False
    return best is None or (value < best if lower else value > best)


def val_line(epoch, n, s):
    """The ``Epoch(val)`` log line of one summary."""
    r, f, o = s['roof'], s['footprint'], s['offset']
    c = s.get('coco') or {}
    tail = ''.join(f', {k}: {c[k]:.4f}' for k in ('bbox_mAP', 'bbox_mAP_50', 'segm_mAP', 'segm_mAP_50') if k in c)
    return (f"Epoch(val) [{epoch}][{n}] roof_F1: {r['F1_score']:.4f}, footprint_F1: {f['F1_score']:.4f}, "
            f"roof_precision: {r['Precision']:.4f}, roof_recall: {r['Recall']:.4f}, footprint_precision: {f['Precision']:.4f}, "
            f"footprint_recall: {f['Recall']:.4f}, aEPE: {o['aEPE']:.4f}, aAE: {o['aAE']:.4f}, pairs: {o['pairs']}" + tail)
