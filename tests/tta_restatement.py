"""torch-CPU restatement of the five test-time-augmentation merges (bonai_amd/csrc/tta.hip), for any of the square's eight symmetries.
tests/test_tta_cpu.py holds it to the reference's own outputs (tests/golden/tta_ops.npz) bit for bit; tests/test_tta_gpu.py holds
the kernels to it.  Element encoding and step order: bonai_amd/tta.py (transpose, x-mirror, y-mirror; back in reverse)."""
import torch

from bonai_amd.kernels import D4_MIRROR_X, D4_MIRROR_Y, D4_TRANSPOSE
from oracle import cops, ops_ref as R


def _dims(e, H, W):
    return (W, H) if e & D4_TRANSPOSE else (H, W)          # (Hv, Wv)


def _mirror(b, lo, size):
    out = b.clone()
    out[..., lo::4] = size - b[..., lo + 2::4]
    out[..., lo + 2::4] = size - b[..., lo::4]
    return out


def _swap(b):
    out = b.clone()
    out[..., 0::2], out[..., 1::2] = b[..., 1::2], b[..., 0::2]
    return out


def boxes_to_view(b, e, H, W):
    Hv, Wv = _dims(e, H, W)
    if e & D4_TRANSPOSE:
        b = _swap(b)
    if e & D4_MIRROR_X:
        b = _mirror(b, 0, Wv)
    if e & D4_MIRROR_Y:
        b = _mirror(b, 1, Hv)
    return b


def boxes_from_view(b, e, H, W):
    Hv, Wv = _dims(e, H, W)
    if e & D4_MIRROR_Y:
        b = _mirror(b, 1, Hv)
    if e & D4_MIRROR_X:
        b = _mirror(b, 0, Wv)
    if e & D4_TRANSPOSE:
        b = _swap(b)
    return b


def mean_views(xs):
    """Sequential fp32 sum in view order divided by V."""
    acc = torch.zeros_like(xs[0])
    for x in xs:
        acc = acc + x
    return acc / float(len(xs))


def view_rois(boxes, elems, H, W):
    n = boxes.shape[0]
    return torch.cat([torch.cat([torch.full((n, 1), float(v)), boxes_to_view(boxes[:, :4], e, H, W)], 1) for v, e in enumerate(elems)], 0)


def gather_proposals(props, counts, elems, H, W):
    out = []
    for v, e in enumerate(elems):
        p = props[v, :int(counts[v])]
        out.append(torch.cat([boxes_from_view(p[:, :4], e, H, W), p[:, 4:5]], 1))
    return torch.cat(out, 0)


def merge_proposals(props, counts, elems, H, W, nms_thr, max_num):
    """merge_aug_proposals: the gathered proposals through the C oracle's nms, best max_num by score."""
    g = gather_proposals(props, counts, elems, H, W)
    dets, _ = cops.nms(g[:, :4].contiguous(), g[:, 4].contiguous(), nms_thr)
    _, order = dets[:, 4].sort(0, descending=True)
    return dets[order[:min(max_num, dets.shape[0])]]


def merge_view_bboxes(view_boxes, view_scores, elems, H, W):
    """merge_aug_bboxes on per-view decoded boxes [V][n,4k] / scores [V][n,C+1]."""
    return mean_views([boxes_from_view(b, e, H, W) for b, e in zip(view_boxes, elems)]), mean_views(list(view_scores))


def merge_bboxes(rois, bbox_pred, cls_score, elems, H, W, means, stds):
    V = len(elems)
    n = rois.shape[0] // V
    vb, vs = [], []
    for v, e in enumerate(elems):
        sl = slice(v * n, (v + 1) * n)
        Hv, Wv = _dims(e, H, W)
        k = bbox_pred.shape[1] // 4
        rr = rois[sl, 1:].repeat_interleave(k, dim=0)
        vb.append(R.delta2bbox(rr, bbox_pred[sl].reshape(-1, 4), means, stds, (Hv, Wv)).view(n, 4 * k))
        vs.append(torch.softmax(cls_score[sl], dim=1))
    return merge_view_bboxes(vb, vs, elems, H, W)


def grid_from_view(m, e):
    """[..., S, S] of a view -> the original frame (merge_aug_masks' mask[..., ::-1] for a flip)."""
    if e & D4_MIRROR_Y:
        m = m.flip(-2)
    if e & D4_MIRROR_X:
        m = m.flip(-1)
    if e & D4_TRANSPOSE:
        m = m.transpose(-1, -2)
    return m


def merge_masks(probs, elems):
    """probs [V,n,S,S] (sigmoid applied) -> merged [n,S,S]."""
    return mean_views([grid_from_view(probs[v], e).contiguous() for v, e in enumerate(elems)])


def paste_views(logits, boxes, elems, img_h, img_w, thr=0.5):
    return R.paste_masks(merge_masks(logits.sigmoid(), elems)[:, None], boxes, img_h, img_w, thr)


def offsets_from_view(o, e):
    if e & D4_MIRROR_Y:
        o = o * torch.tensor([1., -1.])
    if e & D4_MIRROR_X:
        o = o * torch.tensor([-1., 1.])
    if e & D4_TRANSPOSE:
        o = o.flip(1)
    return o


def merge_offsets_foa(pred, rois, elems, stds=(0.5, 0.5), max_shape=(1024, 1024)):
    """pred [4, V n, 2] branch-major (one run of the FOA head over the view-major RoIs)."""
    V = len(elems)
    n = rois.shape[0] // V
    if n == 0:
        return pred.new_zeros(0, 2)
    p4 = pred.view(4, V, n, 2)
    outs = []
    for v, e in enumerate(elems):
        fused = R.foa_fuse(p4[:, v].reshape(4 * n, 2))
        ms = (max_shape[1], max_shape[0]) if e & D4_TRANSPOSE else max_shape
        outs.append(offsets_from_view(R.delta2offset(rois[v * n:(v + 1) * n, 1:], fused, stds=stds, max_shape=ms), e))
    return mean_views(outs)
