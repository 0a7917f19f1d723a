"""GPU: test-time augmentation (bonai_amd/csrc/tta.hip, bonai_amd/tta.py, LOFT.aug_test).  The kernels are held to the torch-CPU
restatement of tests/tta_restatement.py, which tests/test_tta_cpu.py holds to the reference's own outputs bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_restatement as T  # noqa: E402
from oracle import ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLIP_VIEWS = {1: [0], 2: [0, 2], 3: [0, 2, 4]}                       # on the 64 x 96 tile: none, horizontal, vertical
ROT_VIEWS = {1: [0], 2: [0, 3], 3: [0, 3, 6], 8: [0, 2, 4, 3, 6, 5, 1, 7]}    # on the 64 x 64 tile: all eight symmetries
# the decoders' bound of tests/test_glue_gpu.py::test_coders (expf of the device against the host's)
CODER = dict(rtol=1e-5, atol=1e-3)
# softmax scores lie in [0, 1]: exp(x - max) <= 1 carries the device expf's error (<= 2 ulp) and the quotient's half ulp per view;
# 16 ulp of 1.0 = 2e-6 covers the mean of up to eight views with room for the host's own differently-rounded expf
SCORE_ATOL = 2e-6


def _cases():
    out = []
    for V in (1, 2, 3, 8):
        if V in FLIP_VIEWS:
            out.append((FLIP_VIEWS[V], 64, 96))
        out.append((ROT_VIEWS[V], 64, 64))
    return out


def _boxes(rng, n, h, w):
    x, y = rng.uniform(-6, w + 2, n), rng.uniform(-6, h + 2, n)
    b = np.stack([x, y, x + rng.uniform(0.5, w / 2, n), y + rng.uniform(0.5, h / 2, n)], 1).astype(np.float32)
    edge = np.array([[0, 0, w, h], [0, 0, 0, 0], [w - 3, h - 5, w, h], [10.5, 20.25, 10.5, 31], [w + 4, h + 1, w + 20, h + 9],
                     [-30, -20, -2, -1]], np.float32)          # borders, zero area, outside the image
    b[:min(n, len(edge))] = edge[:n]
    return torch.from_numpy(b)


@pytest.mark.parametrize('n', [0, 1, 65, 300])
def test_kernels_match_the_restatement(n):
    from bonai_amd import kernels as K
    rng = np.random.RandomState(100 + n)
    for elems, H, W in _cases():
        V = len(elems)
        table = K.tta_view_table(elems, 'cuda')
        boxes = _boxes(rng, n, H, W)
        rois = K.tta_view_rois(boxes.cuda(), table, V, H, W)
        want_rois = T.view_rois(boxes, elems, H, W)
        assert rois.shape == (V * n, 5) and torch.equal(rois.cpu(), want_rois), (elems, 'view_rois')
        # proposals: P = n slots per view, one view with count 0
        P = max(n, 1)
        props = torch.cat([torch.stack([_boxes(rng, P, H, W) for _ in range(V)]), torch.from_numpy(rng.rand(V, P, 1).astype(np.float32))], 2)
        counts = torch.from_numpy(rng.randint(0, n + 1, V).astype(np.int64))
        counts[V // 2] = 0
        got = K.tta_gather_proposals(props.cuda(), counts.cuda(), table, H, W)
        assert torch.equal(got.cpu(), T.gather_proposals(props, counts, elems, H, W)), (elems, 'gather_proposals')
        for C in (1, 3):
            for Cb in {C, 1}:
                bp = torch.from_numpy(rng.randn(V * n, 4 * Cb).astype(np.float32))
                cs = torch.from_numpy((rng.randn(V * n, C + 1) * 3).astype(np.float32))
                means, stds = (0., 0., 0., 0.), (.1, .1, .2, .2)
                gb, gs = K.tta_merge_bboxes(want_rois.cuda(), bp.cuda(), cs.cuda(), V, table, H, W, means, stds)
                wb, ws = T.merge_bboxes(want_rois, bp, cs, elems, H, W, means, stds)
                assert gb.shape == (n, 4 * Cb) and gs.shape == (n, C + 1)
                assert torch.allclose(gb.cpu(), wb.view(n, 4 * Cb), **CODER), (elems, C, Cb)
                assert torch.allclose(gs.cpu(), ws, rtol=0, atol=SCORE_ATOL), (elems, C)
        pred = torch.from_numpy(rng.randn(4 * V * n, 2).astype(np.float32))
        go = K.tta_merge_offsets(pred.cuda(), want_rois.cuda(), V, table, max_shape=(40, 48))
        wo = T.merge_offsets_foa(pred, want_rois, elems, max_shape=(40, 48))
        assert go.shape == (n, 2) and torch.allclose(go.cpu(), wo.view(n, 2), **CODER), (elems, 'merge_offsets')


def _paste_inputs(V, N=12, S=28, H=128, W=160, seed=3):
    rng = np.random.RandomState(seed)
    logits = torch.from_numpy((rng.randn(V, N, S, S) * 3).astype(np.float32))
    cx, cy = rng.uniform(0, W, N), rng.uniform(0, H, N)
    w, h = rng.uniform(8, 120, N), rng.uniform(8, 100, N)
    boxes = torch.tensor(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1), dtype=torch.float32)
    boxes[0] = torch.tensor([-20., -10., 60., 50.])            # partly outside
    boxes[1] = torch.tensor([150., 100., 190., 140.])          # over the far corner
    return logits, boxes, H, W


@pytest.mark.parametrize('elems', [[0], [0, 2], [0, 2, 4], [0, 2, 4, 3, 6, 5, 1, 7]])
def test_paste_views_vs_oracle_paste_of_the_merged_probabilities(elems):
    """The existing paste test's condition (tests/test_inference_gpu.py:50-52): at most 2e-4 of the pixels differ from
    oracle.ops_ref.paste_masks on the merged probabilities; boxes >= 8 px wide on a 128 x 160 canvas.  The restatement alone stays
    inside that share against a float64 evaluation of the same merge (checked here on the CPU for this seed)."""
    from bonai_amd import kernels as K
    V = len(elems)
    logits, boxes, H, W = _paste_inputs(V)
    ref = T.paste_views(logits, boxes, elems, H, W, 0.5)
    merged64 = torch.stack([T.grid_from_view(logits[v].double().sigmoid(), e) for v, e in enumerate(elems)]).mean(0)
    ref64 = R.paste_masks(merged64[:, None].float(), boxes, H, W, 0.5)
    share64 = (ref != ref64).float().mean().item()
    got = K.mask_paste_views(logits.cuda(), boxes.cuda(), K.tta_view_table(elems, 'cuda'), H, W, 0.5).bool().cpu()
    share = (got != ref).float().mean().item()
    print(f'V={V}: kernel vs restatement {share:.2e}, restatement vs float64 merge {share64:.2e}')
    assert share64 < 2e-4
    assert share < 2e-4


@pytest.mark.parametrize('H,W', [(96, 128), (50, 70), (33, 16)])
def test_paste_views_of_one_identity_view_is_mask_paste_bit_for_bit(H, W):
    from bonai_amd import kernels as K
    logits, boxes, _, _ = _paste_inputs(1, H=H, W=W, seed=5)
    boxes[2] = torch.tensor([10., 10., 10., 40.])              # zero-width box -> inf handling
    a = K.mask_paste(logits[0].cuda(), boxes.cuda(), H, W, 0.5)
    b = K.mask_paste_views(logits.cuda(), boxes.cuda(), K.tta_view_table([0], 'cuda'), H, W, 0.5)
    assert a.shape == b.shape and torch.equal(a, b)
    assert K.mask_paste_views(logits[:, :0].cuda(), boxes[:0].cuda(), K.tta_view_table([0], 'cuda'), H, W).shape == (0, H, W)


@pytest.mark.parametrize('V', [2, 4])
def test_identical_identity_views_give_the_single_view_value_bit_for_bit(V):
    """A power-of-two mean of equal terms is exact (not asserted for V = 3).  The view table is built by hand: equal views are
    not a view list bonai_amd.tta would make."""
    from bonai_amd import kernels as K
    rng = np.random.RandomState(9)
    n, H, W, C = 65, 64, 96, 3
    table = torch.zeros(V, dtype=torch.int32, device='cuda')
    one = K.tta_view_table([0], 'cuda')
    boxes = _boxes(rng, n, H, W).cuda()
    r1, rv = K.tta_view_rois(boxes, one, 1, H, W), K.tta_view_rois(boxes, table, V, H, W)
    assert torch.equal(rv[:, 1:], r1[:, 1:].repeat(V, 1))
    bp, cs = torch.randn(n, 4 * C, device='cuda'), torch.randn(n, C + 1, device='cuda') * 3
    means, stds = (0., 0., 0., 0.), (.1, .1, .2, .2)
    b1, s1 = K.tta_merge_bboxes(r1, bp, cs, 1, one, H, W, means, stds)
    bv, sv = K.tta_merge_bboxes(rv, bp.repeat(V, 1), cs.repeat(V, 1), V, table, H, W, means, stds)
    assert torch.equal(b1, bv) and torch.equal(s1, sv)
    assert torch.equal(b1, K.delta2bbox(r1[:, 1:].repeat_interleave(C, 0), bp.reshape(-1, 4), means, stds, (H, W)).view(n, -1))
    pred = torch.randn(4, n, 2, device='cuda')
    o1 = K.tta_merge_offsets(pred.reshape(-1, 2), r1, 1, one)
    ov = K.tta_merge_offsets(pred[:, None].expand(4, V, n, 2).reshape(-1, 2), rv, V, table)
    assert torch.equal(o1, ov) and torch.equal(o1, K.foa_fuse_decode(pred.reshape(-1, 2), r1[:, 1:]))
    p3 = torch.randn(n, 3, device='cuda')
    q1 = K.tta_merge_offsets(p3, r1, 1, one, foa=False, polar=True)
    assert torch.equal(q1, K.offset_decode(p3, r1[:, 1:], polar=True))
    assert torch.equal(q1, K.tta_merge_offsets(p3.repeat(V, 1), rv, V, table, foa=False, polar=True))
    logits, mb, Hm, Wm = _paste_inputs(1)
    assert torch.equal(K.mask_paste_views(logits.cuda(), mb.cuda(), one, Hm, Wm),
                       K.mask_paste_views(logits.repeat(V, 1, 1, 1).cuda(), mb.cuda(), table, Hm, Wm))


def _write_dataset(tmp_path, n_tiles=2, size=64):
    from PIL import Image
    rng = np.random.RandomState(1)
    images = []
    for i in range(n_tiles):
        name = f't{i}.png'
        Image.fromarray(rng.randint(0, 255, (size, size, 3)).astype(np.uint8)).save(tmp_path / name, compress_level=1)
        images.append(dict(id=i + 1, file_name=name, width=size, height=size))
    f = tmp_path / 'ann.json'
    json.dump(dict(images=images, annotations=[], categories=[dict(id=1, name='building')]), open(f, 'w'))
    return str(f)


def test_all_view_images_come_from_one_launch(tmp_path, monkeypatch):
    from bonai_amd import kernels as K
    from bonai_amd.data import d4_apply
    from bonai_amd.dataset import BonaiDataset
    from bonai_amd.tta import META_KEY, view_element
    f = _write_dataset(tmp_path)
    views = [None, 'horizontal', 'vertical', 90, 180, 270]
    ds = BonaiDataset(f, str(tmp_path), test_mode=True, img_scale=(64, 64), test_views=views)
    calls = []
    real = K.image_prep_d4
    monkeypatch.setattr(K, 'image_prep_d4', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = list(ds.test_batches())
    assert len(out) == 2 and len(calls) == 2                                  # one launch per tile, whatever V
    plain = list(BonaiDataset(f, str(tmp_path), test_mode=True, img_scale=(64, 64)).test_batches())
    for (_, b), (_, p) in zip(out, plain):
        assert len(b['img']) == len(views) and len(b['img_metas']) == len(views)
        base = b['img'][0].cpu().numpy()
        assert np.array_equal(base, p['img'][0].cpu().numpy())               # view 0 is today's image
        for v, op in enumerate(views):
            meta = b['img_metas'][v][0]
            assert meta[META_KEY] == view_element(op) and meta['flip'] == isinstance(op, str)
            assert meta['rotate_angle'] == (op if isinstance(op, int) else 0)
            assert np.array_equal(b['img'][v].cpu().numpy(), d4_apply(base, view_element(op), axes=(2, 3)))


def _model(fp32=False, **rcnn):
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    cfg.test_cfg.rcnn.update(rcnn)
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    m = m.cuda().eval()
    if fp32:
        m.backbone.compute_dtype = torch.float32
    return m


def _views_of(data, ops):
    from bonai_amd.data import d4_apply
    from bonai_amd.tta import view_element, view_meta
    img = data['img'].cpu().numpy()
    imgs = [torch.from_numpy(np.ascontiguousarray(d4_apply(img, view_element(op), axes=(2, 3)))).cuda() for op in ops]
    return imgs, [[view_meta(data['img_metas'][0], op)] for op in ops]


def test_aug_test_fp32_parity_mode_vs_reference_fixture():
    """The reference's own aug_test on three views (none / horizontal / vertical) of the seeded 256^2 tile, tests/golden/tta_256.npz,
    against LOFT.aug_test in the fp32 parity mode at the bounds of test_simple_test_fp32_parity_mode_vs_reference_fixture: score 1e-4,
    box 5e-3 px, mask area 8 px.  Offsets: shape, dtype and finiteness only (the reference returns none)."""
    from bonai_amd.synth import make_batch
    gd = np.load(os.path.join(ROOT, 'tests', 'golden', 'tta_256.npz'))
    size = int(gd['meta'][0])
    m = _model(fp32=True)
    imgs, metas = _views_of(make_batch(1, size, 4, device='cuda'), [None, 'horizontal', 'vertical'])
    with torch.no_grad():
        bbox_results, segm_results, offset_results = m(img=imgs, img_metas=metas, return_loss=False, rescale=True)
    tol_s, tol_b, tol_area = 1e-4, 5e-3, 8
    det, want = torch.from_numpy(bbox_results[0]), torch.from_numpy(gd['det'])
    assert offset_results.dtype == np.float32 and offset_results.shape == (det.shape[0], 2) and np.isfinite(offset_results).all()
    assert det.shape == want.shape
    ds = (det[:, 4] - want[:, 4]).abs().max().item()
    dbox = (want[:, None, :4] - det[None, :, :4]).abs().amax(-1)
    dbox = torch.where((want[:, None, 4] - det[None, :, 4]).abs() < tol_s, dbox, torch.full_like(dbox, 1e9))
    best, arg = dbox.min(1)
    areas = torch.tensor([int(s.sum()) for s in segm_results[0]])[arg]
    da = (areas - torch.from_numpy(gd['mask_area'])).abs().max().item()
    print(f'aug_test fp32 parity mode: score max diff {ds:.2e}, box max diff {best.max().item():.2e} px, mask area max diff {da} px')
    assert ds < tol_s
    assert best.max().item() < tol_b, best.max().item()
    assert da <= tol_area


def test_aug_test_bf16_tuple_rle_and_empty():
    from bonai_amd import rle as RL
    from bonai_amd.synth import make_batch
    m = _model()
    data = make_batch(1, 256, 4, device='cuda')
    imgs, metas = _views_of(data, [None, 'horizontal', 'vertical', 90])
    with torch.no_grad():
        bbox_results, segm, offsets = m(img=imgs, img_metas=metas, return_loss=False, rescale=True)
        m.roi_head.test_cfg['rle_masks'] = True
        b2, segm_rle, o2 = m(img=imgs, img_metas=metas, return_loss=False, rescale=True)
    n = bbox_results[0].shape[0]
    assert isinstance(bbox_results, list) and len(bbox_results) == 1 and bbox_results[0].shape[1] == 5 and n > 0
    assert bbox_results[0].dtype == np.float32 and len(segm[0]) == n and offsets.shape == (n, 2) and offsets.dtype == np.float32
    assert segm[0][0].dtype == np.bool_ and segm[0][0].shape == (256, 256) and np.isfinite(offsets).all()
    assert np.array_equal(b2[0], bbox_results[0]) and np.array_equal(o2, offsets) and len(segm_rle[0]) == n
    for r, b in list(zip(segm_rle[0], segm[0]))[:100]:
        assert r['size'] == [256, 256] and np.array_equal(RL.rle_decode(r), b)
    m.roi_head.test_cfg['rle_masks'] = False
    m.roi_head.test_cfg['score_thr'] = 2.0                       # nothing passes: the empty forms of simple_test
    with torch.no_grad():
        e_aug = m(img=imgs, img_metas=metas, return_loss=False, rescale=True)
        e_one = m(img=imgs[:1], img_metas=metas[:1], return_loss=False, rescale=True)
    assert e_aug[0][0].shape == (0, 5) and e_aug[1] == e_one[1] == [[]] and e_aug[2] == e_one[2]


def test_one_view_still_takes_simple_test_and_training_is_untouched(monkeypatch):
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    from oracle.synth_weights import synth_tensor
    m = _model()
    data = make_batch(1, 256, 4, device='cuda')
    called = []
    monkeypatch.setattr(type(m), 'aug_test', lambda self, *a, **k: called.append(1))
    with torch.no_grad():
        got = m(img=[data['img']], img_metas=[data['img_metas']], return_loss=False, rescale=True)
        want = m.simple_test(data['img'], data['img_metas'], rescale=True)
    assert not called and np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[2], want[2])
    assert all(np.array_equal(a, b) for a, b in zip(got[1][0], want[1][0]))
    monkeypatch.undo()

    # a training step after a TTA pass reproduces the step without it -- the rule of
    # tests/test_validate_gpu.py::test_training_is_undisturbed_by_a_validation_pass: within 4x the largest difference between TWO
    # PLAIN runs (the atomics' summation order), floor one fp32 ulp of the value; bit-identical if the plain runs are
    from bonai_amd import kernels as K
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    batch = make_batch(2, 256, 4, device='cuda')

    def step(with_tta):
        torch.manual_seed(0)
        t = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        t.load_state_dict({k: synth_tensor(k, v.shape) for k, v in t.state_dict().items()})
        t = t.cuda()
        if with_tta:
            t.eval()
            imgs, metas = _views_of(data, [None, 'horizontal', 90])
            with torch.no_grad():
                t(img=imgs, img_metas=metas, return_loss=False, rescale=True)
        t.train()
        K._SAMPLE_CALLS[0] = 0
        out = t.train_step(batch)
        out['loss'].backward()
        torch.cuda.synchronize()
        grads = torch.cat([p.grad.float().reshape(-1)[:64] for _, p in sorted(t.named_parameters()) if p.grad is not None])
        return np.concatenate([[out['loss'].item()], grads.double().cpu().numpy()]), int(K._SAMPLE_CALLS[0])
    (xa, ca), (xb, cb), (xc, cc) = step(False), step(False), step(True)
    assert ca == cb == cc and xa.shape == xc.shape
    spread, got = float(np.abs(xa - xb).max()), np.abs(xa - xc)
    print(f'plain-vs-plain spread {spread:.3e}, after-TTA-vs-plain max {float(got.max()):.3e}')
    if spread == 0.0:
        assert np.array_equal(xa, xc)
    else:
        assert np.all(got <= np.maximum(4 * spread, np.spacing(np.abs(xa).astype(np.float32)).astype(np.float64)))
