"""GPU: kernels.mask_paste_rle (bonai_amd/csrc/mask_rle.hip) -- COCO RLE strings straight from the mask logits -- against the path
it replaces, which stays in the tree: rle.rle_encode_masks of the bitmaps of kernels.mask_paste / mask_paste_views / mask_translate.
Equality is on the bytes of every detection of every case; nothing is sampled and nothing has a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_rle_restatement as M  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(h, w, S, names=None):
    tn, boxes, logits = M.table(h, w, S)
    keep = [i for i, n in enumerate(tn) if names is None or n in names]
    return [tn[i] for i in keep], torch.from_numpy(boxes[keep]).cuda(), torch.from_numpy(logits[keep]).cuda()


def _same(fused, bitmaps, h, w):
    """fused strings == the reference's strings of the bitmaps, and they decode to the bitmaps; -> the reference's strings."""
    from bonai_amd import rle as RL
    ref = RL.rle_encode_masks(bitmaps)
    assert len(fused) == len(ref) == bitmaps.shape[0]
    host = bitmaps.bool().cpu().numpy()
    for i, (f, r) in enumerate(zip(fused, ref)):
        assert f['size'] == r['size'] == [h, w] and isinstance(f['counts'], bytes)
        assert f['counts'] == r['counts'], (i, f['counts'][:40], r['counts'][:40])
        assert np.array_equal(RL.rle_decode(f), host[i]), i
    return ref, host


@pytest.mark.parametrize('thr', [0.5, 0.3])
@pytest.mark.parametrize('S', [28, 14])
@pytest.mark.parametrize('h, w', [(37, 29), (130, 70)])
def test_table_bytes_equal_the_bitmap_path(h, w, S, thr):
    from bonai_amd import kernels as K
    names, boxes, logits = _table(h, w, S)
    ref, host = _same(K.mask_paste_rle(logits, boxes, h, w, thr), K.mask_paste(logits, boxes, h, w, thr), h, w)
    by = dict(zip(names, ref))
    assert by['cover_hi']['counts'] == b'0' + _chars(h * w) and by['interior_lo']['counts'] == _chars(h * w)
    seen = set()
    for r, m in zip(ref, host):
        seen |= M.kinds(r['counts'], m)
    assert seen >= M.ALL_KINDS - {'four_chars'}, seen              # a four-character count needs 2^14 pixels: the 1024^2 case


def _chars(c):
    from bonai_amd import rle as RL
    return RL.counts_to_string([c])


def test_1024_tile_four_detections_and_every_kind():
    from bonai_amd import kernels as K
    h = w = 1024
    names, boxes, logits = M.big_table(28, h)
    boxes, logits = torch.from_numpy(boxes).cuda(), torch.from_numpy(logits).cuda()
    assert len(names) == 4
    ref, host = _same(K.mask_paste_rle(logits, boxes, h, w, 0.5), K.mask_paste(logits, boxes, h, w, 0.5), h, w)
    seen = set()
    for r, m in zip(ref, host):
        seen |= M.kinds(r['counts'], m)
    assert seen == M.ALL_KINDS, seen
    lead, chars = M.string_fields(ref[names.index('interior_smooth')]['counts'])[0]
    assert 4.5e5 < lead < 6e5 and chars >= 4                       # a leading run of about 5e5: four characters or more


def test_no_detections():
    from bonai_amd import kernels as K
    assert K.mask_paste_rle(torch.zeros(0, 28, 28, device='cuda'), torch.zeros(0, 4, device='cuda'), 37, 29) == []
    assert K.mask_paste_rle(torch.zeros(3, 0, 28, 28, device='cuda'), torch.zeros(0, 4, device='cuda'), 64, 64,
                            views=K.tta_view_table([0, 2, 4], 'cuda'), offsets=torch.zeros(0, 2, device='cuda')) == []


def _random(n, h, w, S, seed, V=None):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([w + 8., h + 8.]) - 8
    boxes = torch.cat([xy, xy + 1 + torch.rand(n, 2, generator=g) * torch.tensor([w * .6, h * .6])], 1)
    logits = torch.randn(*((n, S, S) if V is None else (V, n, S, S)), generator=g) * 3
    return boxes.cuda(), logits.cuda()


def test_300_random_boxes_and_the_capacity_path():
    from bonai_amd import kernels as K
    h, w, n = 130, 70, 300
    boxes, logits = _random(n, h, w, 28, 0)
    fused = K.mask_paste_rle(logits, boxes, h, w, 0.5)
    _same(fused, K.mask_paste(logits, boxes, h, w, 0.5), h, w)
    # buffers far too small: the kernel reports what it needs, writes nothing past them, and the one retry gives the same bytes;
    # then a capacity that fits (one read back), and one where only the bytes are short
    need_runs = sum(len(M.string_fields(f['counts'])) for f in fused)
    need_bytes = sum(len(f['counts']) for f in fused)
    for cap in ((16, 32), (need_runs, need_bytes), (need_runs, need_bytes // 2), (need_runs // 3, need_bytes)):
        assert K.mask_paste_rle(logits, boxes, h, w, 0.5, capacity=cap) == fused, cap


@pytest.mark.parametrize('elems, h, w', [([0, 2, 4], 130, 70), ([0, 2, 3, 5], 64, 64)])
def test_views_equal_mask_paste_views(elems, h, w):
    from bonai_amd import kernels as K
    table = K.tta_view_table(elems, 'cuda')
    for S, thr in ((28, 0.5), (14, 0.3)):
        boxes, logits = _random(40, h, w, S, 1, V=len(elems))
        names, tb, tl = _table(h, w, S)
        boxes = torch.cat([boxes, tb])
        logits = torch.cat([logits, torch.stack([tl.roll(v, 0) for v in range(len(elems))])], 1).contiguous()
        _same(K.mask_paste_rle(logits, boxes, h, w, thr, views=table), K.mask_paste_views(logits, boxes, table, h, w, thr), h, w)


@pytest.mark.parametrize('h, w', [(37, 29), (130, 70)])
def test_footprints_equal_mask_translate_of_the_roof(h, w):
    from bonai_amd import kernels as K
    names, boxes, logits = _table(h, w, 28)
    i = names.index('interior_smooth')
    offs = [(0, 0), (3.4, -2.6), (2.5, -2.5), (-7, 5), (w * .5, 3), (w + 3, -h), (-2.5, 2.5), (0.4, h * .5), (-w * 2, 0), (0, h * 3.)]
    for off in offs:                                          # every table row under every offset
        o = torch.tensor([off], dtype=torch.float32).repeat(len(names), 1).cuda()
        roofs = K.mask_paste(logits, boxes, h, w, 0.5)
        feet = K.mask_translate(roofs, o)
        ref, host = _same(K.mask_paste_rle(logits, boxes, h, w, 0.5, offsets=o), feet, h, w)
        if off == (2.5, -2.5):                                # halves round away from zero: 3 and -3
            assert np.array_equal(host[i], M.translate_np(roofs[i].bool().cpu().numpy(), (3, -3)))
        if off == (w * .5, 3):
            assert 0 < host[i].sum() < int(roofs[i].sum())    # partly out of the image
        if off == (w + 3, -h):
            assert ref[i]['counts'] == _chars(h * w)          # wholly out
    # one offset per detection, with views
    table = K.tta_view_table([0, 2, 4], 'cuda')
    boxes, logits = _random(60, h, w, 14, 2, V=3)
    o = (torch.rand(60, 2, generator=torch.Generator().manual_seed(3)) * 40 - 20).cuda()
    feet = K.mask_translate(K.mask_paste_views(logits, boxes, table, h, w, 0.3), o)
    _same(K.mask_paste_rle(logits, boxes, h, w, 0.3, views=table, offsets=o), feet, h, w)


def test_argument_limits_are_errors():
    from bonai_amd import kernels as K, lib as L
    z = torch.zeros(1, 28, 28, device='cuda')
    b = torch.tensor([[1., 1., 9., 9.]], device='cuda')
    with pytest.raises(L.LoftHipError):
        K.mask_paste_rle(torch.zeros(1, 65, 65, device='cuda'), b, 64, 64)          # S > 64
    with pytest.raises(L.LoftHipError):
        K.mask_paste_rle(z, b, 2 ** 19, 2 ** 12)                                    # img_h * img_w = 2^31
    with pytest.raises(L.LoftHipError):
        K.mask_paste_rle(torch.zeros(2, 1, 28, 28, device='cuda'), b, 64, 64)       # views without their table


def _model(**rcnn):
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    cfg.test_cfg.rcnn.update(rcnn)
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    return m.cuda().eval()


def _model_level(m, imgs, metas):
    from bonai_amd import kernels as K, rle as RL
    cfg = m.roi_head.test_cfg

    def run(**kw):
        for k in ('rle_masks', 'footprint_rle'):
            cfg.pop(k, None)
        cfg.update(kw)
        with torch.no_grad():
            return m(img=imgs, img_metas=metas, return_loss=False, rescale=True)
    bitmap = run()
    rle = run(rle_masks=True)
    fused = run(rle_masks='fused')
    feet = run(rle_masks='fused', footprint_rle=True)
    assert len(bitmap) == len(rle) == len(fused) == 3 and len(feet) == 4
    n = bitmap[0][0].shape[0]
    assert n > 0 and len(rle[1][0]) == n
    assert fused[1] == rle[1] and feet[1] == rle[1]                               # dict content and order
    for r in (rle, fused, feet):
        assert np.array_equal(r[0][0], bitmap[0][0]) and np.array_equal(r[2], bitmap[2])
    roofs = torch.from_numpy(np.stack(bitmap[1][0])).cuda()
    want = K.mask_translate(roofs, torch.from_numpy(np.asarray(feet[2], np.float32)).cuda())
    assert len(feet[3]) == len(feet[1]) == 1 and len(feet[3][0]) == n
    assert feet[3][0] == RL.rle_encode_masks(want)
    assert np.array_equal(RL.rle_decode(feet[3][0][0]), want[0].bool().cpu().numpy())
    cfg['score_thr'] = 2.0                                                        # nothing passes: the empty forms
    with torch.no_grad():
        e = m(img=imgs, img_metas=metas, return_loss=False, rescale=True)
    assert len(e) == 4 and e[1] == [[]] and e[3] == [[]]
    cfg['keep_device_masks'] = True
    with pytest.raises(ValueError, match='keep_device_masks'):
        m(img=imgs, img_metas=metas, return_loss=False, rescale=True)


def test_simple_test_fused_results_equal_the_bitmap_path():
    from bonai_amd.synth import make_batch
    data = make_batch(1, 256, 4, device='cuda')
    _model_level(_model(), [data['img']], [data['img_metas']])


def test_aug_test_fused_results_equal_the_bitmap_path():
    from bonai_amd.data import d4_apply
    from bonai_amd.synth import make_batch
    from bonai_amd.tta import view_element, view_meta
    data = make_batch(1, 256, 4, device='cuda')
    ops = [None, 'horizontal', 'vertical', 90]
    img = data['img'].cpu().numpy()
    imgs = [torch.from_numpy(np.ascontiguousarray(d4_apply(img, view_element(op), axes=(2, 3)))).cuda() for op in ops]
    _model_level(_model(), imgs, [[view_meta(data['img_metas'][0], op)] for op in ops])
