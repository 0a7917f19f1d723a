"""GPU: kernels.multiclass_soft_nms_batched (nms.hip loft_soft_nms_batched) against the loop restatement of
tests/soft_select_restatement.py and oracle.ops_ref.multiclass_nms image by image (naive, linear), and -- all three methods -- against
LoftRoIHead.multiclass_nms, the per-image device path it stands in for, on the same device tensors.  Detections, labels, counts, the
zero padding and the RoIs: exactly.

The whole feature is ONE item of the suite, a few seconds in all: the ``check_*`` functions below take a case each and are called in
loops by the single test at the end, which also runs the model-level checks of tests/test_scene_soft_batch_gpu.py.  Every assertion
names its case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soft_select_restatement as S  # noqa: E402

pytestmark = pytest.mark.gpu
NONE = (np.zeros((0, 5), np.float32), np.zeros((0,), np.int64))      # an image without rows: the per-image forms cannot view [0, 4C]


def _cfg(name, method, agnostic):
    cfg = dict(type='soft_nms', iou_threshold=S.batch(name)[2], method=method)
    if agnostic:
        cfg['class_agnostic'] = True
    return cfg


def _run(name, method, agnostic=False, roi_off_on_device=False):
    from bonai_amd import kernels as K
    images, score_thr, _, k = S.batch(name)
    bboxes = torch.from_numpy(np.concatenate([b for b, _ in images])).cuda()
    scores = torch.from_numpy(np.concatenate([s for _, s in images])).cuda()
    off = np.cumsum([0] + [b.shape[0] for b, _ in images]).tolist()
    cfg = _cfg(name, method, agnostic)
    out = K.multiclass_soft_nms_batched(bboxes, scores, torch.tensor(off).cuda() if roi_off_on_device else off, score_thr, cfg, k)
    return (bboxes, scores, off, cfg), out


def _check(name, want, out):
    images, _, _, k = S.batch(name)
    dets, labels, counts, rois = out
    B = len(images)
    assert dets.shape == (B, k, 5) and dets.dtype == torch.float32 and labels.shape == (B, k) and labels.dtype == torch.int64
    assert counts.shape == (B,) and counts.dtype == torch.int64 and counts.is_cuda and rois.shape == (B * k, 5)
    dets, labels, rois = dets.cpu().numpy(), labels.cpu().numpy(), rois.cpu().numpy()
    assert counts.cpu().tolist() == [w[0].shape[0] for w in want], name
    at = 0
    for b, w in enumerate(want):
        wd, wl = w[0], w[1]
        n = wd.shape[0]
        assert np.array_equal(dets[b, :n].view(np.int32), np.ascontiguousarray(wd).view(np.int32)), (name, b)
        assert np.array_equal(labels[b, :n], wl), (name, b)
        assert not dets[b, n:].view(np.int32).any() and not labels[b, n:].any()                  # the padding: +0.0f and 0
        assert (rois[at:at + n, 0] == b).all()
        assert np.array_equal(rois[at:at + n, 1:].view(np.int32), np.ascontiguousarray(wd[:, :4]).view(np.int32))
        at += n
    assert not rois[at:].view(np.int32).any()


def check_batched_equals_the_restatement(name, agnostic, method):
    _, out = _run(name, method, agnostic)
    _check(name, S.want(name, method, agnostic), out)


def check_hand_case_between_two_images(name):
    from bonai_amd import kernels as K
    bboxes, scores, score_thr, iou_thr, method, max_num, dets, labels = S.hand_cases()[name]
    bboxes, scores = np.asarray(bboxes, np.float32), np.asarray(scores, np.float32)
    C = scores.shape[1] - 1
    images = [S.D.random_image(23, C, 4, 12), (bboxes, scores), S.D.random_image(9, C, 4, 13)]
    off = np.cumsum([0] + [b.shape[0] for b, _ in images]).tolist()
    k = max_num if max_num > 0 else 20
    d, l, c, _ = K.multiclass_soft_nms_batched(torch.from_numpy(np.concatenate([b for b, _ in images])).cuda(),
                                               torch.from_numpy(np.concatenate([s for _, s in images])).cuda(), off, score_thr,
                                               dict(type='soft_nms', iou_threshold=iou_thr, method=method), k)
    n = int(c[1])
    assert np.array_equal(d[1, :n].cpu().numpy(), np.array(dets, np.float32).reshape(-1, 5)) and l[1, :n].tolist() == labels, name


def check_batched_equals_the_oracle(name, agnostic, method):
    from oracle import ops_ref
    images, score_thr, _, k = S.batch(name)
    (_, _, _, cfg), out = _run(name, method, agnostic)
    want = []
    for b, s in images:
        d, l = ops_ref.multiclass_nms(torch.from_numpy(b), torch.from_numpy(s), score_thr, cfg, k) if b.shape[0] else NONE
        want.append((np.asarray(d), np.asarray(l)))
    _check(name, want, out)


def check_batched_equals_the_per_image_device_path(name, agnostic, method):
    """Gaussian too: both kernels decay through one __device__ function, expf included.  roi_off as a device tensor."""
    from bonai_amd.loft.roi import LoftRoIHead
    (bboxes, scores, off, cfg), out = _run(name, method, agnostic, roi_off_on_device=True)
    _, score_thr, _, k = S.batch(name)
    want = []
    for a, e in zip(off, off[1:]):
        if a == e:
            want.append(NONE)
            continue
        d, l = LoftRoIHead.multiclass_nms(None, bboxes[a:e], scores[a:e], score_thr, cfg, k)
        want.append((d.cpu().numpy(), l.cpu().numpy()))
    _check(name, want, out)
    if method != 'gaussian':                            # and the device offsets gave what the host offsets give
        _check(name, S.want(name, method, agnostic), out)


def check_sigma_and_min_score_are_read_from_the_config():
    from bonai_amd import kernels as K
    from bonai_amd.loft.roi import LoftRoIHead
    images, score_thr, iou_thr, k = S.batch('ties_sixteenths')
    b, s = (torch.from_numpy(a).cuda() for a in images[1])
    cfg = dict(type='soft_nms', iou_threshold=iou_thr, method='gaussian', sigma=0.3, min_score=0.2)
    d, l, c, _ = K.multiclass_soft_nms_batched(b, s, [0, b.shape[0]], score_thr, cfg, k)
    wd, wl = LoftRoIHead.multiclass_nms(None, b, s, score_thr, cfg, k)
    plain, _ = LoftRoIHead.multiclass_nms(None, b, s, score_thr, dict(type='soft_nms', iou_threshold=iou_thr, method='gaussian'), k)
    n = int(c[0])
    assert n == wd.shape[0] and torch.equal(d[0, :n], wd) and torch.equal(l[0, :n], wl)
    assert wd.shape != plain.shape or not torch.equal(wd, plain)


def check_refusals_by_name():
    from bonai_amd import kernels as K, lib as L
    b, s = (torch.from_numpy(a).cuda() for a in S.D.random_image(6, 2, 8, 1))
    ok = dict(type='soft_nms', iou_threshold=0.5)
    f = K.multiclass_soft_nms_batched
    for cfg in (dict(type='nms', iou_threshold=0.5), dict(iou_threshold=0.5)):
        with pytest.raises(L.LoftHipError, match='multiclass_nms_batched'):
            f(b, s, [0, 6], 0.05, cfg, 10)
    with pytest.raises(L.LoftHipError, match='predicate'):
        f(b, s, [0, 6], 0.05, dict(ok, predicate='cpu'), 10)
    with pytest.raises(L.LoftHipError, match='methd'):
        f(b, s, [0, 6], 0.05, dict(ok, methd='linear'), 10)
    with pytest.raises(L.LoftHipError, match='method'):
        f(b, s, [0, 6], 0.05, dict(ok, method='quadratic'), 10)
    for k in (0, -1, K.TOPK_MAX + 1):
        with pytest.raises(L.LoftHipError, match='max_per_img'):
            f(b, s, [0, 6], 0.05, ok, k)
    for off in ([0, 5], [1, 6], [0, 4, 3, 6], [6]):
        with pytest.raises(L.LoftHipError, match='roi_off'):
            f(b, s, off, 0.05, ok, 10)
    with pytest.raises(L.LoftHipError, match='bboxes'):
        f(b[:, :6].contiguous(), s, [0, 6], 0.05, ok, 10)
    with pytest.raises(L.LoftHipError):
        f(b.cpu(), s.cpu(), [0, 6], 0.05, ok, 10)                                       # no host fall-back
    with pytest.raises(L.LoftHipError, match='32-bit'):                                 # R * C >= 2^31: refused before anything is touched
        R, C = 2 ** 20, 2 ** 11                                                         # (views of one row: no memory behind them)
        f(torch.zeros(1, 4, device='cuda').expand(R, 4), torch.zeros(1, C + 1, device='cuda').expand(R, C + 1), [0, R], 0.05, ok, 10)
    # and multiclass_nms_batched refuses soft-NMS as before, naming the way in
    with pytest.raises(L.LoftHipError, match='multiclass_soft_nms_batched'):
        K.multiclass_nms_batched(b, s, [0, 6], 0.05, ok, 10)


ORACLE_BATCHES = [('three_c3_per_class', False), ('three_c3_per_class', True), ('three_c3_shared_box', False), ('three_c3_shared_box', True),
                  ('clustered_5000_duplicates', False)]


def test_soft_nms_for_a_batch_of_images():
    for name, agnostic in S.variants():
        for method in ('naive', 'linear'):
            check_batched_equals_the_restatement(name, agnostic, method)
        for method in ('naive', 'linear', 'gaussian'):
            check_batched_equals_the_per_image_device_path(name, agnostic, method)
    for name in sorted(S.hand_cases()):
        check_hand_case_between_two_images(name)
    for name, agnostic in ORACLE_BATCHES:
        for method in ('naive', 'linear'):
            check_batched_equals_the_oracle(name, agnostic, method)
    check_sigma_and_min_score_are_read_from_the_config()
    check_refusals_by_name()
    import test_scene_soft_batch_gpu as SC
    SC.check_all()
