"""GPU: kernels.mask_pair_counts (loft_mask_pair_counts_u8, eval_pairs.hip) -- every prediction x ground-truth pixel intersection
of one image and all areas in one launch -- against the code it replaces in evaluate_image: evaluation._intersections (one slice +
AND + sum per prediction) and ``flatten(1).sum(1)``, on the same device tensors.  Integers: exact equality everywhere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bern(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < 0.5).to(torch.uint8).cuda()


def _check(pm, gm, win, gbox=None):
    from bonai_amd import evaluation as E, kernels as K
    inter, ap, ag = K.mask_pair_counts(pm, gm, win, gbox)
    want = E._intersections(pm, gm, np.asarray(win))
    assert inter.dtype == ap.dtype == ag.dtype == torch.int32
    assert inter.shape == (pm.shape[0], gm.shape[0]) and ap.shape == (pm.shape[0],) and ag.shape == (gm.shape[0],)
    assert torch.equal(inter.long(), want)
    assert torch.equal(ap.long(), pm.flatten(1).sum(1)) and torch.equal(ag.long(), gm.flatten(1).sum(1))
    return inter, ap, ag


def test_window_edge_cases_small_unaligned_image():
    """40x72 (W is no multiple of 16: the byte path), P = 5 sets of windows against G = 7: full image, odd x0 with width 1, height
    1, sticking out past each of the four borders, empty, wholly outside."""
    H, W, G = 40, 72, 7
    gm = _bern((G, H, W), 1)
    groups = [
        [(0, 0, W, H), (13, 3, 14, 30), (5, 17, 60, 18), (-9, 4, 20, 31), (50, 2, W + 11, 20)],
        [(3, -7, 33, 12), (8, 25, 41, H + 9), (-5, -5, W + 5, H + 5), (30, 10, 30, 20), (30, 10, 25, 20)],
        [(10, 20, 40, 20), (10, 20, 40, 12), (-30, 5, -2, 20), (W, 0, W + 20, H), (5, H + 1, 30, H + 9)],
        [(5, -20, 30, 0), (-40, -40, -1, -1), (71, 39, 72, 40), (0, 0, 1, 1), (15, 0, 17, H)],
    ]
    for k, wins in enumerate(groups):
        pm = _bern((5, H, W), 10 + k)
        inter, _, _ = _check(pm, gm, np.asarray(wins, np.int32))
        if k == 0:
            assert torch.equal(inter[0].long(), (gm & pm[0:1]).flatten(1).sum(1))          # the full window is the plain AND count
    assert int(inter[1].sum()) == 0                                                      # (last group: wholly outside -> zeros)


@pytest.fixture(scope='module')
def mid():
    """128x192, P = 67, G = 130: more than one chunk of ground truths and more than 64 of either, neither a multiple of 64; random
    windows of 1..70 pixels a side at unaligned offsets; some all-ones masks on both sides."""
    H, W, P, G = 128, 192, 67, 130
    pm, gm = _bern((P, H, W), 2), _bern((G, H, W), 3)
    pm[[0, 31, 66]] = 1
    gm[[0, 64, 129]] = 1
    rng = np.random.RandomState(5)
    x0, y0 = rng.randint(-10, W - 1, P), rng.randint(-10, H - 1, P)
    win = np.stack([x0, y0, x0 + rng.randint(1, 71, P), y0 + rng.randint(1, 71, P)], 1).astype(np.int32)
    # ground truths confined to boxes, so that a gbox has something to cull (three stay all-ones / unconfined)
    gx0, gy0 = rng.randint(0, W - 20, G), rng.randint(0, H - 20, G)
    ext = np.stack([gx0, gy0, np.minimum(gx0 + rng.randint(5, 90, G), W), np.minimum(gy0 + rng.randint(5, 70, G), H)], 1)
    for g in range(G):
        if g in (0, 64, 129):
            ext[g] = (0, 0, W, H)
            continue
        m = torch.zeros(H, W, dtype=torch.uint8, device='cuda')
        m[ext[g, 1]:ext[g, 3], ext[g, 0]:ext[g, 2]] = 1
        gm[g] &= m
    return pm, gm, win, ext.astype(np.int32)


def test_many_pairs_random_windows(mid):
    pm, gm, win, _ = mid
    inter, _, _ = _check(pm, gm, win)
    assert int(inter.max()) > 0


def test_gbox_cull_never_changes_a_result(mid):
    """gbox at the exact extents, absent, and looser than the extents: three identical results."""
    pm, gm, win, ext = mid
    none = _check(pm, gm, win)
    exact = _check(pm, gm, win, ext)
    loose = _check(pm, gm, win, ext + np.asarray([-7, -3, 9, 40], np.int32))
    for a, b, c in zip(none, exact, loose):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_tile_size_counts_need_32_bits():
    """1024x1024, all ones, full windows: every count is 2^20 -- a 16-bit (or fp16 / bf16) partial sum anywhere would show."""
    from bonai_amd import kernels as K
    pm = torch.ones(3, 1024, 1024, dtype=torch.uint8, device='cuda')
    gm = torch.ones(2, 1024, 1024, dtype=torch.uint8, device='cuda')
    win = np.asarray([[0, 0, 1024, 1024]] * 3, np.int32)
    inter, ap, ag = _check(pm, gm, win)
    assert torch.equal(inter, torch.full((3, 2), 1 << 20, dtype=torch.int32, device='cuda'))
    assert int(ap.min()) == int(ag.min()) == 1 << 20
    again = K.mask_pair_counts(pm, gm, win)                 # no atomics: the same integers from run to run
    assert torch.equal(again[0], inter)


def test_empty_sides_return_empty_outputs():
    from bonai_amd import kernels as K
    some = _bern((4, 40, 72), 7)
    none = some[:0]
    inter, ap, ag = K.mask_pair_counts(none, some, np.zeros((0, 4), np.int32))
    assert inter.shape == (0, 4) and ap.shape == (0,) and ag.shape == (4,) and inter.dtype == torch.int32
    inter, ap, ag = K.mask_pair_counts(some, none, np.asarray([[0, 0, 72, 40]] * 4, np.int32))
    assert inter.shape == (4, 0) and ap.shape == (4,) and ag.shape == (0,)
    inter, ap, ag = K.mask_pair_counts(none, none, np.zeros((0, 4), np.int32))
    assert inter.shape == (0, 0) and ap.shape == (0,) and ag.shape == (0,)


def test_every_output_element_is_written(mid):
    """Outputs pre-filled with 0x7f bytes come back fully overwritten (the caller does not zero them): also for pairs the cull
    skips and for empty windows."""
    from bonai_amd import kernels as K
    pm, gm, win, ext = mid
    win = win.copy()
    win[5] = (20, 20, 20, 40)                               # an empty window
    win[6] = (500, 500, 520, 520)                           # wholly outside
    P, G = pm.shape[0], gm.shape[0]
    out = torch.full((P * G + P + G + 3,), 0x7f7f7f7f, dtype=torch.int32, device='cuda')
    inter, ap, ag = K.mask_pair_counts(pm, gm, win, ext, out=out)
    ref = _check(pm, gm, win, ext)
    assert torch.equal(inter, ref[0]) and torch.equal(ap, ref[1]) and torch.equal(ag, ref[2])
    assert inter.data_ptr() == out.data_ptr() and int((out[:P * G + P + G] == 0x7f7f7f7f).sum()) == 0
    assert int((out[P * G + P + G:] != 0x7f7f7f7f).sum()) == 0          # and nothing past its own elements


def test_polygon_boxes_contain_the_rasterised_pixels():
    """evaluation.polygon_boxes (the gbox evaluate_image derives on the host) contains every set pixel of kernels.poly2mask's
    bitmap, which is what the cull relies on: vertices on and between pixel centres, slanted edges, a polygon leaving the image."""
    from bonai_amd import evaluation as E, kernels as K
    inst = [[[1, 1, 4, 1, 4, 3, 1, 3]], [[10.3, 20.7, 100.2, 30.1, 90.9, 110.4, 15.5, 95.0]], [[49.5, 49.5, 60.5, 49.5, 60.5, 60.5, 49.5, 60.5]],
            [[-3, -3, 12.49, -3, 12.49, 9.51, -3, 9.51]], [[100, 100, 127.9, 100, 127.9, 127.9, 100, 127.9], [5, 90, 30, 90, 17, 120]]]
    m = K.poly2mask(inst, 128, 128)
    box = E.polygon_boxes(inst)
    for i in range(len(inst)):
        ys, xs = torch.nonzero(m[i], as_tuple=True)
        assert ys.numel() and int(xs.min()) >= box[i, 0] and int(xs.max()) < box[i, 2] and int(ys.min()) >= box[i, 1] and int(ys.max()) < box[i, 3]
