"""COCO bbox / segm AP on the device: what the reference's ``evaluation = dict(metric=['bbox', 'segm'])`` asks of
CocoDataset.evaluate (mmdet/datasets/coco.py:364-545), i.e. COCOeval's evaluate / accumulate / summarize, without pycocotools.

pycocotools is not installed here: this module follows the PUBLISHED cocoapi source (PythonAPI/pycocotools/cocoeval.py,
common/maskApi.c) and has NOT been run against it.  tests/coco_eval_restatement.py restates the same source loop for loop in
numpy, tests/test_coco_eval_cpu.py pins that restatement with hand-derived answers, and tests/test_coco_eval_gpu.py holds the
device path to it exactly (bit-equal float64).

Per image (``CocoEvaluator.add_image``): the stable descending score sort and the cut to ``proposal_nums[-1]`` (host: a few hundred
numbers that are host data already), the IoUs (kernels.coco_box_iou; kernels.poly2mask of the annotations' ``segmentation`` +
kernels.mask_pair_counts + kernels.coco_mask_iou) and, several images per launch, the greedy matching of evaluateImg for all area
ranges and IoU thresholds (kernels.coco_match).  What leaves the device per detection is two 64-bit words.  ``summarize`` sorts
all records of a category once (kernels.segmented_sort_desc) and accumulates precision / recall in one launch
(kernels.coco_accumulate); only the means of COCOeval.summarize are taken on the host.

Ground truth is ALL annotations of an image whose category the dataset knows (``bbox``, ``area``, ``iscrowd``), as COCOeval sees
them -- not the filtered set of dataset.parse_bonai_annotations.  A detection's area is w*h (bbox) or its pixel count (segm), as
COCO.loadRes sets it.  Extensions and limits: several shards' records can be merged (``merge_records`` / ``gather_records``);
'proposal' and classwise tables are not built; ``segmentation`` must be polygons (an RLE crowd region raises)."""
import numpy as np
import torch

from . import kernels as K

METRIC_NAMES = ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l')
_A = len(K.COCO_AREA_RNG)


def xyxy2xywh(row):
    """CocoDataset.xyxy2xywh (coco.py:170-189): Python floats of the fp32 values, the differences taken in float64."""
    b = [float(v) for v in row[:4]]
    return [b[0], b[1], b[2] - b[0], b[3] - b[1]]


def stats_from(precision, recall, iou_thrs, max_dets):
    """COCOeval._summarizeDets on precision [T,R,K,A,M] / recall [T,K,A,M] -> the 12 unrounded stats.  cocoapi's own quirk is
    kept: entry 0 reads maxDets == 100 (the default argument), entries 1-5 and 8-11 maxDets[2], entries 6 / 7 maxDets[0] / [1];
    an entry whose maxDets value is not in the list, or whose IoU threshold is not among iou_thrs, is -1."""
    iou_thrs, md = np.asarray(iou_thrs, np.float64), list(max_dets)

    def one(ap, thr=None, a=0, dets=100):
        if dets not in md:
            return -1.0
        s = (precision if ap else recall)[..., a, md.index(dets)]
        if thr is not None:
            s = s[np.where(thr == iou_thrs)[0]]
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    last = md[2] if len(md) > 2 else None
    at = lambda i: md[i] if len(md) > i else None
    return [one(1), one(1, .5, 0, last), one(1, .75, 0, last), one(1, None, 1, last), one(1, None, 2, last), one(1, None, 3, last),
            one(0, None, 0, at(0)), one(0, None, 0, at(1)), one(0, None, 0, last), one(0, None, 1, last), one(0, None, 2, last),
            one(0, None, 3, last)]


def merge_records(parts):
    """The records() of several shards -> one set in image-id order (detections by image ordinal, category, rank), so that the
    stable global score sort breaks ties as a single process does."""
    out = {}
    for metric in parts[0]:
        det = np.concatenate([np.asarray(p[metric]['det'], np.int64).reshape(-1, 6) for p in parts])
        npig = np.concatenate([np.asarray(p[metric]['npig'], np.int64).reshape(-1, 2 + _A) for p in parts])
        out[metric] = dict(det=det[np.lexsort((det[:, 2], det[:, 1], det[:, 0]))], npig=npig[np.lexsort((npig[:, 1], npig[:, 0]))])
    return out


def gather_records(rec, rank, world, device=None):
    """All shards' records on every rank: one MAX all-reduce of the lengths, then one all-gather of the records padded to the
    longest (gloo on host tensors, nccl on device ones, as validate.reduce_counts does) -> merge_records of them."""
    import torch.distributed as dist
    metrics = sorted(rec)
    on_dev = dist.get_backend() == 'nccl'
    put = (lambda t: t.to(device)) if on_dev else (lambda t: t)
    lens = torch.tensor([rec[m][k].shape[0] for m in metrics for k in ('det', 'npig')], dtype=torch.int64)
    flat = torch.from_numpy(np.concatenate([np.asarray(rec[m][k], np.int64).reshape(-1) for m in metrics for k in ('det', 'npig')]))
    size = put(torch.tensor([flat.numel()], dtype=torch.int64))
    dist.all_reduce(size, op=dist.ReduceOp.MAX)
    mine = torch.zeros(lens.numel() + int(size.cpu()[0]), dtype=torch.int64)
    mine[:lens.numel()] = lens
    mine[lens.numel():lens.numel() + flat.numel()] = flat
    mine = put(mine)
    got = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(got, mine)
    parts = []
    for g in got:
        g = g.cpu().numpy()
        n, o, part = g[:lens.numel()], lens.numel(), {}
        for j, m in enumerate(metrics):
            nd, ng = int(n[2 * j]), int(n[2 * j + 1])
            part[m] = dict(det=g[o:o + 6 * nd].reshape(nd, 6), npig=g[o + 6 * nd:o + 6 * nd + (2 + _A) * ng].reshape(ng, 2 + _A))
            o += 6 * nd + (2 + _A) * ng
        parts.append(part)
    return merge_records(parts)


class CocoEvaluator:
    """COCO AP of a detector's results on ``dataset`` (anything with BonaiDataset's ``data_infos`` (id, width, height), ``anns``
    (the raw annotation dicts per image) and ``cat_ids``; label l is category cat_ids[l]).

        ev = CocoEvaluator(ds, metrics=('bbox', 'segm'))
        ev.add_image(i, dets [n,5] (x1, y1, x2, y2, score; host), labels [n], device_masks uint8 [n,H,W])    # every image once
        ev.summarize() -> {'bbox_mAP': ..., ..., 'segm_mAP_copypaste': '...', 'stats': {'bbox': [12 floats], 'segm': [...]}}

    ``mask_windows`` of add_image: int [n,4] half-open pixel windows that contain each detection's set pixels (default: the
    whole image); they only save reads.  ``batch_images``: images queued per matching launch."""

    def __init__(self, dataset, metrics=('bbox', 'segm'), proposal_nums=(100, 300, 1000), iou_thrs=None, batch_images=8,
                 device='cuda'):
        self.metrics = tuple(metrics)
        bad = [m for m in self.metrics if m not in ('bbox', 'segm')]
        if bad or not self.metrics:
            raise ValueError(f"CocoEvaluator: metric {bad[0] if bad else metrics!r} is not 'bbox' or 'segm'")
        self.max_dets = [int(v) for v in proposal_nums]
        if len(set(self.max_dets)) != len(self.max_dets) or not self.max_dets:
            raise ValueError(f'CocoEvaluator: proposal_nums {proposal_nums!r} must be distinct numbers')
        # the fp64 values np.linspace gives (coco.py:409-411, cocoeval.py Params.setDetParams): uploaded, never recomputed
        self.iou_thrs = (np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thrs is None
                         else np.asarray(iou_thrs, np.float64).reshape(-1))
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        if _A * len(self.iou_thrs) > 64 or not 1 <= len(self.iou_thrs) <= K.COCO_MAX_THRS:
            raise ValueError(f'CocoEvaluator: {len(self.iou_thrs)} IoU thresholds x {_A} area ranges do not fit 64 bits per detection')
        self.dataset, self.device, self.batch_images = dataset, device, max(1, int(batch_images))
        self.cats = sorted(set(dataset.cat_ids))
        ids = sorted(set(info['id'] for info in dataset.data_infos))
        self.img_ord = {v: i for i, v in enumerate(ids)}
        self.reset()

    def reset(self):
        self._queue = {m: [] for m in self.metrics}
        self._det = {m: [] for m in self.metrics}
        self._npig = {m: [] for m in self.metrics}
        self._merged = None

    # ---------------------------------------------------------------- per image
    def add_image(self, idx, dets, labels, device_masks=None, mask_windows=None):
        info, anns = self.dataset.data_infos[idx], self.dataset.anns[idx]
        H, W = int(info['height']), int(info['width'])
        dets = np.asarray(dets, np.float32).reshape(-1, 5)
        labels = np.asarray(labels).reshape(-1).astype(np.int64)
        cat_of = np.asarray([self.dataset.cat_ids[int(l)] for l in labels], np.int64) if labels.size else np.zeros(0, np.int64)
        if 'segm' in self.metrics and dets.shape[0]:
            if device_masks is None or tuple(device_masks.shape) != (dets.shape[0], H, W):
                raise ValueError(f"CocoEvaluator('segm'): uint8 device masks [{dets.shape[0]}, {H}, {W}] expected, got "
                                 f'{None if device_masks is None else tuple(device_masks.shape)}')
        if mask_windows is not None:
            mask_windows = np.asarray(mask_windows).reshape(-1, 4)
        for k, cat in enumerate(self.cats):
            gt = [a for a in anns if a['category_id'] == cat]
            sel = np.where(cat_of == cat)[0]
            if not gt and not sel.size:
                continue                                         # (evaluateImg returns None: the image does not count)
            sel = sel[np.argsort(-dets[sel, 4], kind='stable')][:self.max_dets[-1]]
            crowd = np.asarray([int(a.get('iscrowd', 0)) for a in gt], np.uint8)
            gt_area = np.asarray([float(a['area']) for a in gt], np.float64)
            seg = dict(img=self.img_ord[info['id']], cat=k, scores=dets[sel, 4].copy(), D=int(sel.size), G=len(gt), gt_area=gt_area,
                       crowd=crowd)
            for metric in self.metrics:
                s = dict(seg)
                if metric == 'bbox':
                    dt = np.asarray([xyxy2xywh(dets[i]) for i in sel], np.float64).reshape(-1, 4)
                    gb = np.asarray([[float(v) for v in a['bbox']] for a in gt], np.float64).reshape(-1, 4)
                    s['ious'] = K.coco_box_iou(dt, gb, crowd, device=self.device)
                    s['det_area'] = torch.from_numpy(dt[:, 2] * dt[:, 3]).to(self.device)
                else:
                    s['ious'], s['det_area'] = self._mask_ious(sel, gt, crowd, device_masks, mask_windows, H, W)
                self._queue[metric].append(s)
        if max(len(q) for q in self._queue.values()) >= self.batch_images * max(1, len(self.cats)):
            self.flush()

    def _mask_ious(self, sel, gt, crowd, device_masks, windows, H, W):
        from .evaluation import polygon_boxes
        dev = device_masks.device if device_masks is not None else torch.device(self.device)
        D, G = int(sel.size), len(gt)
        for a in gt:
            if not isinstance(a.get('segmentation'), (list, tuple)):
                raise NotImplementedError(f"annotation {a.get('id')}: 'segmentation' is not a polygon list (RLE regions are not read)")
        pm = device_masks[torch.as_tensor(sel, device=dev)].contiguous() if D else torch.zeros(0, H, W, dtype=torch.uint8, device=dev)
        polys = K.pack_polygons([a['segmentation'] for a in gt])
        gm = K.poly2mask(polys, H, W, device=dev) if G else torch.zeros(0, H, W, dtype=torch.uint8, device=dev)
        win = windows[sel] if windows is not None else np.tile(np.asarray([0, 0, W, H]), (D, 1))
        win = np.clip(np.asarray(win, np.float64), -2.0 ** 30, 2.0 ** 30).astype(np.int32)
        inter, area_p, area_g = K.mask_pair_counts(pm, gm, win, polygon_boxes(polys) if G else None)
        return K.coco_mask_iou(inter, area_p, area_g, crowd), area_p.double()

    def flush(self):
        """Match everything queued: one launch per metric."""
        for metric, q in self._queue.items():
            if not q:
                continue
            _, bits, npig = K.coco_match([s['ious'] for s in q], [s['D'] for s in q], [s['G'] for s in q],
                                         torch.cat([s['det_area'].reshape(-1) for s in q]), np.concatenate([s['gt_area'] for s in q]),
                                         np.concatenate([s['crowd'] for s in q]), self.iou_thrs)
            bits, npig, o = bits.cpu().numpy(), npig.cpu().numpy().astype(np.int64), 0
            for j, s in enumerate(q):
                D = s['D']
                rows = np.empty((D, 6), np.int64)
                rows[:, 0], rows[:, 1], rows[:, 2] = s['img'], s['cat'], np.arange(D)
                rows[:, 3] = s['scores'].astype(np.float32).view(np.int32)
                rows[:, 4:] = bits[o:o + D]
                o += D
                self._det[metric].append(rows)
                self._npig[metric].append(np.concatenate([[s['img'], s['cat']], npig[j]]).astype(np.int64).reshape(1, 2 + _A))
            q.clear()

    # ---------------------------------------------------------------- records
    def records(self):
        """{metric: dict(det int64 [N,6] = (image ordinal in sorted image-id order, category ordinal, in-image rank, the fp32
        score's bits, matched word, ignored word), npig int64 [I,2+A] = (image ordinal, category ordinal, non-ignored ground
        truths per area range))} of the images added so far, in image-id order."""
        self.flush()
        own = {m: dict(det=np.concatenate(self._det[m] + [np.zeros((0, 6), np.int64)]),
                       npig=np.concatenate(self._npig[m] + [np.zeros((0, 2 + _A), np.int64)])) for m in self.metrics}
        return merge_records([own])

    def load_records(self, rec):
        """Use ``rec`` (merge_records / gather_records of all shards) instead of this evaluator's own records."""
        self._merged = rec

    # ---------------------------------------------------------------- dataset totals
    def accumulate(self, metric):
        """-> (precision [T,R,K,A,M], recall [T,K,A,M]) float64 host arrays of COCOeval.accumulate."""
        rec = (self._merged if self._merged is not None else self.records())[metric]
        T, R, Kc, M = len(self.iou_thrs), len(self.rec_thrs), len(self.cats), len(self.max_dets)
        precision, recall = -np.ones((T, R, Kc, _A, M)), -np.ones((T, Kc, _A, M))
        for k in range(Kc):
            det = rec['det'][rec['det'][:, 1] == k]
            npig = rec['npig'][rec['npig'][:, 1] == k][:, 2:].sum(0)
            p, r = K.coco_accumulate(torch.from_numpy(det[:, 3].astype(np.int32).view(np.float32).copy()).to(self.device),
                                     det[:, 4:], det[:, 2].astype(np.int32), npig, self.max_dets, self.rec_thrs, T)
            precision[:, :, k], recall[:, k] = p.cpu().numpy(), r.cpu().numpy()
        return precision, recall

    def summarize(self, log=None):
        out, stats = {}, {}
        for metric in self.metrics:
            precision, recall = self.accumulate(metric)
            st = stats_from(precision, recall, self.iou_thrs, self.max_dets)
            stats[metric] = st
            for i, name in enumerate(METRIC_NAMES):
                out[f'{metric}_{name}'] = float(f'{st[i]:.3f}')
            out[f'{metric}_mAP_copypaste'] = ' '.join(f'{v:.3f}' for v in st[:6])
            if log is not None:
                log(f'Evaluating {metric}...')
                for line in summary_lines(st, self.max_dets, self.iou_thrs):
                    log(line)
        out['stats'] = stats
        return out


def summary_lines(stats, max_dets, iou_thrs):
    """The twelve lines COCOeval.summarize prints."""
    md = list(max_dets)
    last = md[2] if len(md) > 2 else -1
    rng = '{:0.2f}:{:0.2f}'.format(iou_thrs[0], iou_thrs[-1])
    rows = [(1, rng, 'all', 100), (1, '0.50', 'all', last), (1, '0.75', 'all', last), (1, rng, 'small', last), (1, rng, 'medium', last),
            (1, rng, 'large', last), (0, rng, 'all', md[0]), (0, rng, 'all', md[1] if len(md) > 1 else -1), (0, rng, 'all', last),
            (0, rng, 'small', last), (0, rng, 'medium', last), (0, rng, 'large', last)]
    return [' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
        'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou, area, dets, v)
        for (ap, iou, area, dets), v in zip(rows, stats)]
