"""LoftRoIHead's inference entry points (simple_test, aug_test, simple_test_device) without a GPU and without the library: every call
that would reach the library is a recording fake, and each case asserts the full trace -- which calls, in which order, with which
shapes and scalars, and where a result is copied to the host -- and the structure of what comes back.

Shapes: 6 proposals, 2 classes, S = 4 mask logits, a 16 x 16 network input, V = 2 views.  The fake NMS keeps 3 detections with the
scores 0.9, 0.6, 0.3 and the labels [1, 0, 1], so per-class grouping and its order are visible.  The mask head's fake writes
10 * row + class into every logit: the class-selected logits name the (row, class) they were taken from.
"""
import types

import numpy as np
import pytest
import torch
from torch import nn

from bonai_amd import kernels as K
from bonai_amd import rle as RLE
from bonai_amd.config import ConfigDict
from bonai_amd.loft import roi as R

NP, NCLS, S, IMG, V = 6, 2, 4, 16, 2
ELEMS = [0, 2]
DETS = [[1., 1., 5., 5., .9], [2., 2., 8., 8., .6], [3., 3., 12., 12., .3]]
LABELS = [1, 0, 1]
KEEP = [1, 0, 3]                      # rows of the [12] candidate list (proposal-major, class-minor): its labels are [1, 0, 1]
NMS = dict(type='nms', iou_threshold=0.5)
MEANS, STDS = (0., 0., 0., 0.), (.1, .1, .2, .2)
MODES = {'bitmaps': {}, 'rle': {'rle_masks': True}, 'fused': {'rle_masks': 'fused'},
         'feet': {'rle_masks': 'fused', 'footprint_rle': True}}


class Traced(torch.Tensor):
    """What the fakes return: a tensor whose copy to the host shows up in the trace."""
    trace = None

    def cpu(self):
        Traced.trace.append(('cpu', tuple(self.shape)))
        return self.as_subclass(torch.Tensor)


def tr(t):
    return t.as_subclass(Traced)


def shp(t):
    return tuple(t.shape)


def bsum(boxes):
    return round(float(boxes.as_subclass(torch.Tensor).sum()), 3)


def ids(logits):
    return logits.as_subclass(torch.Tensor)[..., 0, 0].reshape(-1).tolist()


class Extractor:
    num_inputs = 1

    def __init__(self, name, trace):
        self.name, self.trace = name, trace

    def __call__(self, feats, rois, n_rot=1):
        self.trace.append((self.name, len(feats), shp(rois), n_rot))
        return tr(torch.zeros(n_rot * rois.shape[0], 2, 3, 3))


def make_head(trace, cfg, with_mask=True, plain_offsets=False):
    head = R.LoftRoIHead.__new__(R.LoftRoIHead)
    nn.Module.__init__(head)
    head.test_cfg = ConfigDict(score_thr=0.0, nms=ConfigDict(NMS), max_per_img=100, mask_thr_binary=0.5, **cfg)
    head.with_mask = with_mask
    head.bbox_roi_extractor = Extractor('bbox_roi_extractor', trace)
    head.mask_roi_extractor = Extractor('mask_roi_extractor', trace)
    head.offset_roi_extractor = Extractor('offset_roi_extractor', trace)

    def decode(rr, bp, max_shape=None):
        trace.append(('decode', shp(rr), shp(bp), tuple(max_shape)))
        return tr(rr.as_subclass(torch.Tensor) + 1)

    def bbox_head(feats):
        trace.append(('bbox_head', shp(feats)))
        n = feats.shape[0]
        return tr(torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) / 10), tr(torch.ones(n, 4 * NCLS))
    bbox_head.num_classes = NCLS
    bbox_head.bbox_coder = types.SimpleNamespace(decode=decode, means=MEANS, stds=STDS)
    head.bbox_head = bbox_head

    def mask_head(feats):
        trace.append(('mask_head', shp(feats)))
        n = feats.shape[0]
        v = 10 * torch.arange(n, dtype=torch.float32)[:, None] + torch.arange(NCLS, dtype=torch.float32)[None]
        return tr(v[:, :, None, None].expand(n, NCLS, S, S).contiguous())
    mask_head.class_agnostic = False
    head.mask_head = mask_head

    cls = R.OffsetHead if plain_offsets else R.OffsetHeadExpandFeature
    oh = cls.__new__(cls)
    nn.Module.__init__(oh)
    oh.offset_coder = types.SimpleNamespace(means=(0., 0.), stds=(.5, .5))
    oh.offset_coordinate = 'rectangle'
    oh.expand_feature_num, oh.rot_idx = 4, (0, 1, 2, 3)

    def offset_forward(x):
        trace.append(('offset_head', shp(x)))
        return tr(torch.ones(x.shape[0], 2))
    if plain_offsets:
        oh.forward = offset_forward
    else:
        oh.forward_rotated = offset_forward
    head.offset_head = oh
    return head


@pytest.fixture
def trace(monkeypatch):
    t = []
    Traced.trace = t

    def batched_nms(boxes, scores, labels, nms_cfg, class_agnostic=False):
        t.append(('batched_nms', shp(boxes), shp(scores), labels.tolist(), dict(nms_cfg)))
        return tr(torch.tensor(DETS)), torch.tensor(KEEP)

    def mask_paste(logits, boxes, img_h, img_w, thr=0.5):
        t.append(('mask_paste', shp(logits), ids(logits), shp(boxes), bsum(boxes), img_h, img_w, thr))
        out = torch.zeros(logits.shape[0], img_h, img_w, dtype=torch.uint8)
        for i in range(out.shape[0]):
            out[i, 0, i] = 1                          # bitmap i has its one pixel in column i
        return tr(out)

    def mask_paste_views(logits, boxes, views, img_h, img_w, thr=0.5):
        t.append(('mask_paste_views', shp(logits), ids(logits), shp(boxes), bsum(boxes), views.tolist(), img_h, img_w, thr))
        out = torch.zeros(logits.shape[1], img_h, img_w, dtype=torch.uint8)
        for i in range(out.shape[0]):
            out[i, 0, i] = 1
        return tr(out)

    def mask_paste_rle(logits, boxes, img_h, img_w, thr=0.5, views=None, offsets=None, capacity=None):
        assert capacity is None
        t.append(('mask_paste_rle', shp(logits), ids(logits), shp(boxes), bsum(boxes), img_h, img_w, thr,
                  None if views is None else views.tolist(), None if offsets is None else (shp(offsets), offsets.dtype)))
        n = logits.shape[-3]
        return [{'size': [img_h, img_w], 'counts': b'%s%d' % (b'roof' if offsets is None else b'foot', i)} for i in range(n)]

    def rle_encode_masks(masks):
        t.append(('rle_encode_masks', shp(masks), masks.dtype))
        return [{'size': list(masks.shape[1:]), 'counts': b'enc%d' % i} for i in range(masks.shape[0])]

    def tta_view_table(elems, device):
        t.append(('tta_view_table', [int(e) for e in elems], str(device)))
        return torch.tensor([int(e) for e in elems], dtype=torch.int32)

    def tta_view_rois(boxes, views, nv, img_h, img_w):
        t.append(('tta_view_rois', shp(boxes), boxes.is_contiguous(), bsum(boxes[:, :4]), views.tolist(), nv, img_h, img_w))
        n = boxes.shape[0]
        b = boxes.as_subclass(torch.Tensor)[:, :4].float()
        return tr(torch.cat([torch.cat([torch.full((n, 1), float(v)), b], 1) for v in range(nv)], 0))

    def tta_merge_bboxes(rois, bbox_pred, cls_score, nv, views, img_h, img_w, means, stds):
        t.append(('tta_merge_bboxes', shp(rois), shp(bbox_pred), shp(cls_score), nv, views.tolist(), img_h, img_w, tuple(means), tuple(stds)))
        n = rois.shape[0] // nv
        return tr(torch.ones(n, bbox_pred.shape[1])), tr(torch.full((n, cls_score.shape[1]), 0.25))

    def tta_merge_offsets(pred, rois, nv, views, means=(0., 0.), stds=(0.5, 0.5), max_shape=(1024, 1024), foa=True, polar=False):
        t.append(('tta_merge_offsets', shp(pred), shp(rois), nv, views.tolist(), tuple(means), tuple(stds), tuple(max_shape), foa, polar))
        n = rois.shape[0] // nv
        return tr(torch.arange(2 * n, dtype=torch.float64).reshape(n, 2))

    def foa_fuse_decode(pred, boxes, stds=(0.5, 0.5), max_shape=(1024, 1024)):
        t.append(('foa_fuse_decode', shp(pred), shp(boxes), boxes.is_contiguous(), bsum(boxes), tuple(stds), tuple(max_shape)))
        n = boxes.shape[0]
        return tr(torch.arange(2 * n, dtype=torch.float64).reshape(n, 2))

    def offset_decode(pred, boxes, means=(0., 0.), stds=(0.5, 0.5), max_shape=(1024, 1024), polar=False):
        t.append(('offset_decode', shp(pred), shp(boxes), boxes.is_contiguous(), bsum(boxes), tuple(means), tuple(stds), tuple(max_shape), polar))
        n = boxes.shape[0]
        return tr(torch.arange(2 * n, dtype=torch.float64).reshape(n, 2))

    for name, fn in dict(batched_nms=batched_nms, mask_paste=mask_paste, mask_paste_views=mask_paste_views, mask_paste_rle=mask_paste_rle,
                         tta_view_table=tta_view_table, tta_view_rois=tta_view_rois, tta_merge_bboxes=tta_merge_bboxes,
                         tta_merge_offsets=tta_merge_offsets, foa_fuse_decode=foa_fuse_decode, offset_decode=offset_decode).items():
        monkeypatch.setattr(K, name, fn)
    monkeypatch.setattr(RLE, 'rle_encode_masks', rle_encode_masks)
    yield t
    Traced.trace = None


def proposals():
    b = torch.arange(NP, dtype=torch.float32)[:, None]
    return torch.cat([b, b, b + 4, b + 4, torch.full((NP, 1), 0.5)], 1)          # sum of the boxes: 108


# ------------------------------------------------------------------ what a case must record and return

def expected_trace(entry, mode, kept, sf=1.0, rescale=False, with_mask=True, plain=False, nodet=False):
    """The calls of one case, in order.  kept: how many of the 3 detections pass paste_min_score; sf: the image's scale factor."""
    aug = entry == 'aug'
    nv = V if aug else 1
    views = ELEMS if aug else None
    t = []
    if aug:
        t += [('tta_view_table', ELEMS, 'cpu'), ('tta_view_rois', (NP, 5), True, 108.0, ELEMS, V, IMG, IMG)]
    t += [('bbox_roi_extractor', 1, (nv * NP, 5), 1), ('bbox_head', (nv * NP, 2, 3, 3))]
    if aug:
        t += [('tta_merge_bboxes', (V * NP, 5), (V * NP, 4 * NCLS), (V * NP, NCLS + 1), V, ELEMS, IMG, IMG, MEANS, STDS)]
    else:
        t += [('decode', (NP * NCLS, 4), (NP * NCLS, 4), (IMG, IMG, 3))]
    if not nodet:
        t += [('batched_nms', (NP * NCLS, 4), (NP * NCLS,), [0, 1] * NP, NMS)]
    else:
        kept = 0
    t += [('cpu', (kept, 5)), ('cpu', (kept,))]              # detections and labels: before the mask head is enqueued
    if kept == 0:
        return t
    raw = sum(sum(d[:4]) for d in DETS[:kept])               # the detections' boxes as NMS returned them
    net = raw * sf if rescale else raw                       # ... in the network input's frame: RoIs and offsets
    side = IMG if aug else (int(IMG / sf) if rescale else IMG)          # the paste's canvas: ori_shape, or ori_shape * scale_factor
    sel = [10. * (v * kept + i) + LABELS[i] for v in range(nv) for i in range(kept)]
    lshape = (V, kept, S, S) if aug else (kept, S, S)
    if aug:
        t += [('tta_view_rois', (kept, 4), True, raw, ELEMS, V, IMG, IMG)]

    def paste_rle(offsets=None):
        return ('mask_paste_rle', lshape, sel, (kept, 4), raw, side, side, 0.5, views, offsets)
    if with_mask:
        t += [('mask_roi_extractor', 1, (nv * kept, 5), 1), ('mask_head', (nv * kept, 2, 3, 3))]
        if mode in ('fused', 'feet'):
            t += [paste_rle()]
        else:
            t += [('mask_paste_views', lshape, sel, (kept, 4), raw, ELEMS, IMG, IMG, 0.5) if aug else
                  ('mask_paste', lshape, sel, (kept, 4), raw, side, side, 0.5)]
            t += [('rle_encode_masks', (kept, side, side), torch.uint8)] if mode == 'rle' else [('cpu', (kept, side, side))]
    t += [('offset_roi_extractor', 1, (nv * kept, 5), 1 if plain else 4), ('offset_head', ((1 if plain else 4) * nv * kept, 2, 3, 3))]
    npred = ((1 if plain else 4) * nv * kept, 2)
    if aug:
        t += [('tta_merge_offsets', npred, (V * kept, 5), V, ELEMS, (0., 0.), (.5, .5), (1024, 1024), not plain, False)]
    elif plain:
        t += [('offset_decode', npred, (kept, 4), True, net, (0., 0.), (.5, .5), (1024, 1024), False)]
    else:
        t += [('foa_fuse_decode', npred, (kept, 4), True, net, (.5, .5), (1024, 1024))]
    t += [('cpu', (kept, 2))]
    if mode == 'feet' and with_mask:
        t += [paste_rle(((kept, 2), torch.float32))]
    return t


def check_result(res, mode, kept, with_mask=True, side=IMG):
    feet = mode == 'feet'
    assert type(res) is tuple and len(res) == (4 if feet else 3)
    bbox, segm, offs = res[:3]
    assert type(bbox) is list and len(bbox) == NCLS
    assert all(type(b) is np.ndarray and b.dtype == np.float32 and b.ndim == 2 and b.shape[1] == 5 for b in bbox)
    by_class = [[i for i in range(kept) if LABELS[i] == c] for c in range(NCLS)]          # detection order kept inside a class
    for c in range(NCLS):
        assert bbox[c].tolist() == np.array([DETS[i] for i in by_class[c]], np.float32).reshape(-1, 5).tolist()
    per_class = ([segm] + ([res[3]] if feet else []))
    if not with_mask:
        assert all(p is None for p in per_class)
    else:
        for p, word in zip(per_class, (b'roof', b'foot')):
            assert type(p) is list and [len(q) for q in p] == [len(b) for b in by_class]
            for c in range(NCLS):
                for r, i in zip(p[c], by_class[c]):
                    if mode == 'bitmaps':
                        assert type(r) is np.ndarray and r.dtype == np.bool_ and r.shape == (side, side)
                        assert r.sum() == 1 and r[0, i]
                    else:
                        want = b'enc%d' % i if mode == 'rle' else word + b'%d' % i
                        assert r == {'size': [side, side], 'counts': want}
    if kept == 0:
        assert offs == [[], []]
    else:
        assert type(offs) is np.ndarray and offs.dtype == np.float32
        assert offs.tolist() == np.arange(2 * kept, dtype=np.float32).reshape(kept, 2).tolist()


def check_last(head, cfg, mode, kept, with_mask=True, side=IMG):
    """last_device_masks / last_dets / last_det_labels: with keep_device_masks, not on the empty return, not with footprints."""
    if not cfg.get('keep_device_masks') or kept == 0 or mode == 'feet':
        assert not any(hasattr(head, a) for a in ('last_device_masks', 'last_dets', 'last_det_labels'))
        return
    if with_mask:
        m = head.last_device_masks
        assert isinstance(m, torch.Tensor) and m.dtype == torch.uint8 and tuple(m.shape) == (kept, side, side)
        assert all(int(m[i].sum()) == 1 and int(m[i, 0, i]) == 1 for i in range(kept))     # bitmap order = detection order
    else:
        assert head.last_device_masks is None
    assert type(head.last_dets) is np.ndarray and head.last_dets.dtype == np.float32
    assert head.last_dets.tolist() == np.array(DETS[:kept], np.float32).tolist()
    assert type(head.last_det_labels) is np.ndarray and head.last_det_labels.dtype == np.int64
    assert head.last_det_labels.tolist() == LABELS[:kept]


def _cases():
    out = []
    for entry in ('simple', 'aug'):
        for mode in MODES:
            out.append(dict(entry=entry, mode=mode))
        for mode in ('bitmaps', 'rle'):
            out.append(dict(entry=entry, mode=mode, keep=True))
        for mode, keep in (('bitmaps', False), ('bitmaps', True), ('feet', False)):
            out.append(dict(entry=entry, mode=mode, keep=keep, pms=0.5))          # drops the third detection
            out.append(dict(entry=entry, mode=mode, keep=keep, pms=0.95))         # drops all of them
            out.append(dict(entry=entry, mode=mode, keep=keep, nodet=True))
        for mode, keep in (('bitmaps', False), ('bitmaps', True), ('rle', False), ('fused', False), ('feet', False)):
            out.append(dict(entry=entry, mode=mode, keep=keep, with_mask=False))
        out.append(dict(entry=entry, mode='bitmaps', with_mask=False, nodet=True))
        out.append(dict(entry=entry, mode='feet', with_mask=False, nodet=True))
        out.append(dict(entry=entry, mode='bitmaps', plain=True))
        out.append(dict(entry=entry, mode='feet', plain=True))
    for mode in MODES:
        out.append(dict(entry='simple', mode=mode, rescale=True))
    out.append(dict(entry='simple', mode='bitmaps', rescale=True, keep=True, pms=0.5))
    out.append(dict(entry='simple', mode='bitmaps', padded=True))
    out.append(dict(entry='simple', mode='feet', padded=True, rescale=True))
    return out


def _id(c):
    return '-'.join([c['entry'], c['mode']] + [k if v is True else f'{k}{v}' for k, v in c.items() if k not in ('entry', 'mode') and v])


@pytest.mark.parametrize('case', _cases(), ids=_id)
def test_simple_test_and_aug_test(case, trace):
    entry, mode = case['entry'], case['mode']
    keep, pms, nodet = case.get('keep', False), case.get('pms'), case.get('nodet', False)
    with_mask, plain, rescale = case.get('with_mask', True), case.get('plain', False), case.get('rescale', False)
    cfg = dict(MODES[mode])
    if keep:
        cfg['keep_device_masks'] = True
    if pms is not None:
        cfg['paste_min_score'] = pms
    head = make_head(trace, cfg, with_mask, plain)
    if nodet:
        head.test_cfg['score_thr'] = 2.0                     # no score passes: NMS is not reached
    kept = 0 if nodet else (3 if pms is None else sum(d[4] >= pms for d in DETS))
    props = proposals()
    if entry == 'simple':
        sf = 2.0
        meta = dict(img_shape=(IMG, IMG, 3), ori_shape=(IMG // 2, IMG // 2, 3), scale_factor=np.full(4, sf, np.float32))
        plist = (torch.cat([props, torch.zeros(2, 5)])[None], torch.tensor([NP])) if case.get('padded') else [props]
        res = head.simple_test([torch.zeros(1, 2, 8, 8)], plist, [meta], rescale=rescale)
        side = IMG // 2 if rescale else IMG
    else:
        sf = 1.0
        meta = dict(img_shape=(IMG, IMG, 3), ori_shape=(IMG, IMG, 3), scale_factor=np.ones(4, np.float32))
        res = head.aug_test([torch.zeros(V, 2, 8, 8)], props, [[meta]] * V, ELEMS)
        side = IMG
    assert trace == expected_trace(entry, mode, kept, sf, rescale, with_mask, plain, nodet)
    check_result(res, mode, kept, with_mask, side)
    check_last(head, cfg, mode, kept, with_mask, side)


def _device_call(head, scale=1.0, padded=False):
    props = proposals()
    meta = dict(img_shape=(IMG, IMG, 3), ori_shape=(IMG, IMG, 3), scale_factor=np.full(4, scale, np.float32))
    plist = (torch.cat([props, torch.zeros(2, 5)])[None], torch.tensor([NP])) if padded else [props]
    return head.simple_test_device([torch.zeros(1, 2, 8, 8)], plist, [meta])


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('plain', [False, True])
def test_simple_test_device(trace, padded, plain):
    head = make_head(trace, {}, plain_offsets=plain)
    det, labels, logits, offsets = _device_call(head, padded=padded)
    raw = sum(sum(d[:4]) for d in DETS)
    nb = 1 if plain else 4
    assert trace == [
        ('bbox_roi_extractor', 1, (NP, 5), 1), ('bbox_head', (NP, 2, 3, 3)), ('decode', (NP * NCLS, 4), (NP * NCLS, 4), (IMG, IMG, 3)),
        ('batched_nms', (NP * NCLS, 4), (NP * NCLS,), [0, 1] * NP, NMS),
        ('mask_roi_extractor', 1, (3, 5), 1), ('mask_head', (3, 2, 3, 3)),
        ('offset_roi_extractor', 1, (3, 5), nb), ('offset_head', (nb * 3, 2, 3, 3)),
        ('offset_decode', (3, 2), (3, 4), True, raw, (0., 0.), (.5, .5), (1024, 1024), False) if plain else
        ('foa_fuse_decode', (12, 2), (3, 4), True, raw, (.5, .5), (1024, 1024))]                    # no copy to the host
    assert all(isinstance(t, torch.Tensor) for t in (det, labels, logits, offsets))
    assert det.tolist() == torch.tensor(DETS).tolist() and labels.tolist() == LABELS and labels.dtype == torch.int64
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (3, S, S)
    assert logits[:, 0, 0].tolist() == [10. * i + LABELS[i] for i in range(3)]
    assert offsets.dtype == torch.float32 and offsets.tolist() == [[0., 1.], [2., 3.], [4., 5.]]
    assert not any(hasattr(head, a) for a in ('last_device_masks', 'last_dets', 'last_det_labels'))


def test_simple_test_device_without_detections(trace):
    head = make_head(trace, {})
    head.test_cfg['score_thr'] = 2.0
    det, labels, logits, offsets = _device_call(head)
    assert trace == [('bbox_roi_extractor', 1, (NP, 5), 1), ('bbox_head', (NP, 2, 3, 3)),
                     ('decode', (NP * NCLS, 4), (NP * NCLS, 4), (IMG, IMG, 3))]
    assert tuple(det.shape) == (0, 5) and tuple(labels.shape) == (0,) and labels.dtype == torch.int64
    assert tuple(logits.shape) == (0, 0, 0) and tuple(offsets.shape) == (0, 2)


def test_simple_test_device_refusals(trace):
    with pytest.raises(ValueError, match='paste_min_score'):
        _device_call(make_head(trace, {'paste_min_score': 0.5}))
    with pytest.raises(NotImplementedError, match='no mask head'):
        _device_call(make_head(trace, {}, with_mask=False))
    with pytest.raises(NotImplementedError, match='scale_factor'):
        _device_call(make_head(trace, {}), scale=2.0)
    assert trace == []                                       # each of them before anything is computed
