"""GPU: whole-scene inference (bonai_amd/scene.py, bonai_amd/csrc/scene.hip).  Tile preparation against image_prep_d4 of the torch
crop, bit for bit; mask areas and pair intersections against integer sums over kernels.mask_paste's bitmaps, exactly; the
suppression against the greedy loop of tests/scene_restatement.py; the detector against simple_test on one tile and against the
restatement's merge of four tiles.  Nothing has a tolerance, and nothing is compared with the code under test."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_restatement as R  # noqa: E402
from test_scene_cpu import GREEDY_CASES  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def _scene_u8(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(H, W, 3, generator=g) * 58 + 120).clamp(0, 255).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- tile preparation
@pytest.mark.parametrize('H, W, overlap', [(70, 50, 32), (97, 130, 32), (50, 40, 0)])
@pytest.mark.parametrize('kept', [False, True])
def test_tile_prep_equals_image_prep_of_the_crop(H, W, overlap, kept):
    from bonai_amd import kernels as K
    from bonai_amd.scene import tile_grid
    t = 64
    scene = _scene_u8(H, W, 7).cuda()
    origins = tile_grid(H, W, t, overlap)
    got = K.scene_tile_prep(scene, torch.from_numpy(origins).cuda(), (t, t), kept, MEAN, STD)
    assert got.shape == (len(origins), 3, t, t) and got.dtype == torch.float32
    padded = 0
    for k, (x0, y0) in enumerate(origins.tolist()):
        h, w = min(t, H - y0), min(t, W - x0)
        crop = torch.full((1, t, t, 3), 201, dtype=torch.uint8, device='cuda')      # what lies outside the scene must not matter
        crop[0, :h, :w] = scene[y0:y0 + h, x0:x0 + w]
        want = K.image_prep_d4(crop, [0], [kept], MEAN, STD)[0]                     # element 0: the identity
        assert torch.equal(got[k, :, :h, :w].view(torch.int32), want[:, :h, :w].view(torch.int32)), (k, x0, y0)
        outside = torch.ones(t, t, dtype=torch.bool, device='cuda')
        outside[:h, :w] = False
        assert int((got[k].view(torch.int32)[:, outside] != 0).sum()) == 0          # +0.0f, bit for bit
        padded += int(outside.any())
    if (H, W) == (97, 130):
        assert len(origins) == 12 and padded == 0 and [33, 66] == [int(origins[-1][1]), int(origins[-1][0])]   # inward-shifted, odd
    else:
        assert padded == len(origins)
    if (H, W) == (50, 40):
        assert len(origins) == 1                                                    # padded both ways


def test_tile_prep_takes_any_origin_table():
    """Origins the grid never makes: tiles hanging over every edge of the scene, and one wholly outside."""
    from bonai_amd import kernels as K
    H, W, t = 37, 53, 64
    scene = _scene_u8(H, W, 8).cuda()
    origins = torch.tensor([[-5, -9], [30, 20], [52, 36], [53, 0], [-64, 0], [3, 1]], dtype=torch.int32).cuda()
    got = K.scene_tile_prep(scene, origins, (t, t), False, MEAN, STD)
    canvas = torch.zeros(1, 3 * t, 3 * t, 3, dtype=torch.uint8, device='cuda')
    canvas[0, t:t + H, t:t + W] = scene
    full = K.image_prep_d4(canvas, [0], [False], MEAN, STD)[0]
    inside = torch.zeros(canvas.shape[1:3], dtype=torch.bool, device='cuda')
    inside[t:t + H, t:t + W] = True
    full = torch.where(inside, full, torch.zeros_like(full))
    for k, (x0, y0) in enumerate(origins.tolist()):
        assert torch.equal(got[k].view(torch.int32), full[:, t + y0:2 * t + y0, t + x0:2 * t + x0].view(torch.int32)), k


# ---------------------------------------------------------------------------------------------------------------- pair counts
def _placed(S=28):
    """About 40 detections on a 97 x 130 canvas over four tile indices -> (boxes [N,4], tiles [N], logits [N,S,S], names)."""
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float32), np.arange(S, dtype=np.float32), indexing='ij')
    c = np.float32(S - 1) / 2
    smooth = (4 - 8 * ((yy - c) ** 2 + (xx - c) ** 2) / np.float32(S / 2) ** 2).astype(np.float32)     # +4 centre, -12 corners
    rows = [
        # the same building seen by two / three tiles
        ('bldg_a0', [12.3, 14.1, 40.2, 44.7], 0), ('bldg_a1', [12.9, 13.6, 40.8, 45.0], 1),
        ('bldg_b0', [60.5, 8.2, 95.1, 30.3], 1), ('bldg_b1', [61.0, 8.0, 94.4, 31.0], 2), ('bldg_b2', [60.1, 9.0, 95.9, 30.0], 3),
        # a roof cut by a tile border next to the whole roof
        ('cut_half', [70.0, 50.2, 86.0, 80.4], 0), ('cut_whole', [70.4, 50.0, 102.2, 80.9], 2),
        # windows [9, 21) x [9, 21) and [21, 31) x [21, 31): they touch at a corner only
        ('corner_a', [10, 10, 20, 20], 0), ('corner_b', [22, 22, 30, 30], 1),
        # windows [39, 51) and [49, 61) in x share two columns, where neither smooth mask has a pixel: a record with inter == 0
        ('strip_a', [40, 60, 50, 70], 2), ('strip_b', [50.5, 60, 60, 70], 3),
        ('zero_width', [110.5, 30, 110.5, 50], 1), ('over_zero_width', [100, 25, 125, 55], 0),
        ('clip_topleft', [-5, -4, 12, 9], 3), ('over_topleft', [-2, -2, 14, 12], 0),
        ('clip_bottomright', [118, 85, 140, 105], 2), ('over_bottomright', [112, 80, 131, 99], 1),
        ('same_tile_a', [20, 70, 45, 92], 3), ('same_tile_b', [22, 72, 47, 94], 3),
        ('one_pixel_wide', [33.2, 60, 34.2, 80], 1), ('over_one_pixel', [25, 58, 40, 82], 0),
        ('outside_scene', [140, 20, 160, 40], 2),
    ]
    rng = np.random.RandomState(5)
    for k in range(18):
        x, y = rng.uniform(-4, 115), rng.uniform(-4, 85)
        rows.append((f'random{k}', [x, y, x + rng.uniform(3, 45), y + rng.uniform(3, 40)], k % 4))
    boxes = np.array([r[1] for r in rows], np.float32)
    tiles = np.array([r[2] for r in rows], np.int32)
    noise = torch.randn(len(rows), S, S, generator=torch.Generator().manual_seed(11)).numpy() * 1.5
    logits = (smooth[None] + noise).astype(np.float32)
    names = [r[0] for r in rows]
    for n in ('strip_a', 'strip_b'):
        logits[names.index(n)] = smooth
    return boxes, tiles, logits, names


@pytest.fixture(scope='module')
def placed():
    from bonai_amd import kernels as K
    H, W = 97, 130
    boxes, tiles, logits, names = _placed()
    db, dt, dl = torch.from_numpy(boxes).cuda(), torch.from_numpy(tiles).cuda(), torch.from_numpy(logits).cuda()
    bitmaps = K.mask_paste(dl, db, H, W, 0.5).bool().cpu().numpy()
    area, recs = R.pair_counts(bitmaps, boxes, tiles)
    return dict(H=H, W=W, boxes=db, tiles=dt, logits=dl, names=names, area=area, recs=recs, bitmaps=bitmaps)


def _record_dict(recs):
    rows = recs.cpu().numpy().tolist()
    out = {(i, j): c for i, j, c in rows}
    assert len(out) == len(rows), 'a pair twice'
    return out


def test_pair_counts_equal_the_bitmap_sums(placed):
    from bonai_amd import kernels as K
    p, nm = placed, placed['names']
    # the inputs are what the issue asks for: masks neither empty nor full, and every hand-placed situation is really there
    want, area = p['recs'], p['area']
    idx = {n: nm.index(n) for n in nm}
    win = R.windows(p['boxes'].cpu().numpy(), p['H'], p['W'])
    full = (win[:, 1] - win[:, 0]) * (win[:, 3] - win[:, 2])
    named = [idx[n] for n in nm if n.startswith(('bldg', 'cut', 'random', 'over', 'same'))]
    assert all(0 < area[n] < full[n] for n in named)
    assert 35 <= len(nm) <= 45 and sorted(set(p['tiles'].cpu().tolist())) == [0, 1, 2, 3]
    assert want[(idx['bldg_a0'], idx['bldg_a1'])] > 0.7 * area[idx['bldg_a0']]
    assert (idx['corner_a'], idx['corner_b']) not in want
    assert want[(idx['strip_a'], idx['strip_b'])] == 0
    assert (idx['same_tile_a'], idx['same_tile_b']) not in want and (p['bitmaps'][idx['same_tile_a']] & p['bitmaps'][idx['same_tile_b']]).any()
    assert area[idx['zero_width']] > 0 and want[(idx['zero_width'], idx['over_zero_width'])] > 0         # the isinf branch sets pixels
    assert want[(idx['clip_topleft'], idx['over_topleft'])] > 0 and want[(idx['clip_bottomright'], idx['over_bottomright'])] > 0
    assert want[(idx['one_pixel_wide'], idx['over_one_pixel'])] > 0
    assert area[idx['outside_scene']] == 0 and not any(idx['outside_scene'] in k for k in want)
    got_area, recs = K.scene_pair_counts(p['logits'], p['boxes'], p['tiles'], p['H'], p['W'], 0.5)
    assert got_area.dtype == torch.int32 and recs.dtype == torch.int32 and recs.shape[1] == 3
    assert got_area.cpu().tolist() == area.tolist()
    got = _record_dict(recs)
    assert sorted(got.items()) == sorted(want.items())                 # complete, each pair once, every count exact
    assert all(i < j for i, j in got)


def test_pair_counts_capacity_of_one_reports_and_retries(placed):
    from bonai_amd import kernels as K, lib as L
    p = placed
    N, S = p['logits'].shape[0], p['logits'].shape[-1]
    recs = torch.full((4, 3), -7, dtype=torch.int32, device='cuda')
    meta = torch.full((2,), -1, dtype=torch.int64, device='cuda')
    area = torch.empty(N, dtype=torch.int32, device='cuda')
    L.check(L.load().loft_scene_pair_counts(L.ptr(p['logits']), L.ptr(p['boxes']), L.ptr(p['tiles']), N, S, p['H'], p['W'], 0.5,
                                            L.ptr(area), L.ptr(recs), 1, L.ptr(meta), L.stream()), 'loft_scene_pair_counts')
    need, short = meta.tolist()
    assert need == len(p['recs']) and short != 0
    first = tuple(recs[0].tolist())
    assert p['recs'][first[:2]] == first[2] and (recs[1:] == -7).all()         # one record, nothing written past the capacity
    assert area.cpu().tolist() == p['area'].tolist()
    _, again = K.scene_pair_counts(p['logits'], p['boxes'], p['tiles'], p['H'], p['W'], 0.5, capacity=1)
    assert sorted(_record_dict(again).items()) == sorted(p['recs'].items())


def test_pair_counts_limits():
    from bonai_amd import kernels as K, lib as L
    z = torch.zeros(0, 28, 28, device='cuda')
    area, recs = K.scene_pair_counts(z, torch.zeros(0, 4, device='cuda'), torch.zeros(0, dtype=torch.int32, device='cuda'), 64, 64)
    assert area.shape == (0,) and recs.shape == (0, 3)
    with pytest.raises(L.LoftHipError, match='65537'):
        K.scene_pair_counts(torch.zeros(65537, 1, 1, device='cuda'), torch.zeros(65537, 4, device='cuda'),
                            torch.zeros(65537, dtype=torch.int32, device='cuda'), 64, 64)
    with pytest.raises(L.LoftHipError):
        K.scene_pair_counts(torch.zeros(1, 65, 65, device='cuda'), torch.zeros(1, 4, device='cuda'),
                            torch.zeros(1, dtype=torch.int32, device='cuda'), 64, 64)                # S > 64


# ---------------------------------------------------------------------------------------------------------------- suppression
def _suppress(recs, area, scores, trunc, thr):
    from bonai_amd import kernels as K
    r = torch.tensor(recs, dtype=torch.int32).reshape(-1, 3).cuda()
    keep = K.scene_suppress(r, torch.tensor(area, dtype=torch.int32).cuda(), torch.tensor(scores, dtype=torch.float32).cuda(),
                            torch.tensor(trunc, dtype=torch.bool).cuda(), thr)
    assert keep.dtype == torch.uint8
    return keep.cpu().numpy().astype(int).tolist()


@pytest.mark.parametrize('name', sorted(GREEDY_CASES))
def test_suppress_hand_cases(name):
    recs, area, scores, trunc, thr, want = GREEDY_CASES[name]
    assert _suppress(recs, area, scores, trunc, thr) == want


def test_suppress_long_chain_takes_a_round_per_link():
    n = 130                                                            # a chain in priority order: every other one survives
    recs = [(k, k + 1, 90) for k in range(n - 1)]
    scores = [1 - k / 200 for k in range(n)]
    assert _suppress(recs[::-1], [100] * n, scores, [False] * n, 0.5) == [1 - k % 2 for k in range(n)]


def test_suppress_random_graph_equals_the_greedy_loop():
    rng = np.random.RandomState(3)
    N, E = 300, 600
    area = rng.randint(0, 500, N)
    area[rng.rand(N) < 0.03] = 0
    scores = np.round(rng.rand(N), 2).astype(np.float32)               # two decimals: many equal scores
    trunc = rng.rand(N) < 0.3
    pairs = set()
    while len(pairs) < E:
        i, j = sorted(rng.randint(0, N, 2).tolist())
        if i != j:
            pairs.add((i, j))
    recs = []
    for i, j in sorted(pairs):
        m = min(area[i], area[j])
        recs.append((i, j, int(m * 0.5) if rng.rand() < 0.2 else int(rng.randint(0, m + 1))))      # a fifth right at the bound
    want = R.greedy(recs, area, scores, trunc, 0.5).astype(int).tolist()
    assert 0.3 * N < sum(want) < N and sum(1 for i, j, c in recs if min(area[i], area[j]) and c > 0.5 * min(area[i], area[j])) > 150
    assert _suppress(recs, area.tolist(), scores.tolist(), trunc.tolist(), 0.5) == want
    order = rng.permutation(len(recs))
    assert _suppress([recs[k] for k in order], area.tolist(), scores.tolist(), trunc.tolist(), 0.5) == want
    one_shot = np.ones(N, bool)                                        # "any better neighbour" is another rule: the graph has chains
    key = lambda n: (bool(trunc[n]), -float(scores[n]), n)             # noqa: E731
    for i, j, c in recs:
        if min(area[i], area[j]) and c > 0.5 * min(area[i], area[j]):
            one_shot[j if key(i) < key(j) else i] = False
    assert one_shot.astype(int).tolist() != want


# ---------------------------------------------------------------------------------------------------------------- the detector
@pytest.fixture(scope='module')
def model():
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    cfg.test_cfg.rcnn.max_per_img = 60           # the synthetic weights fill any limit: 240 detections keep the restatement quick
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    return m.cuda().eval()


def _meta(h, w):
    return dict(img_shape=(h, w, 3), pad_shape=(h, w, 3), ori_shape=(h, w, 3), scale_factor=np.ones(4, np.float32), flip=False)


def test_one_tile_scene_equals_simple_test_fused(model):
    from bonai_amd import kernels as K
    from bonai_amd.scene import SceneDetector
    scene = _scene_u8(256, 256, 21)
    res = SceneDetector(model, tile=256, overlap=128, footprints=True).run(scene.numpy())
    img = K.image_prep_d4(scene.cuda()[None], [0], [False], MEAN, STD)
    cfg = model.roi_head.test_cfg
    cfg.update(rle_masks='fused', footprint_rle=True)
    try:
        with torch.no_grad():
            want = model(img=[img], img_metas=[[_meta(256, 256)]], return_loss=False, rescale=True)
    finally:
        cfg.pop('rle_masks'), cfg.pop('footprint_rle')
    n = want[0][0].shape[0]
    assert n > 0 and len(res) == n
    assert np.array_equal(res.bboxes, want[0][0]) and res.bboxes.dtype == np.float32
    assert np.array_equal(res.offsets, want[2]) and (res.labels == 0).all() and (res.tiles == 0).all()
    assert res.roofs == want[1][0] and res.footprints == want[3][0]                  # dicts: sizes and bytes
    got = res.as_result_tuple()
    assert len(got) == 4 and np.array_equal(got[0][0], want[0][0]) and got[1] == want[1] and got[3] == want[3]
    assert np.array_equal(got[2], want[2])


def test_four_tile_scene_equals_the_restatement_merge(model):
    from bonai_amd import kernels as K, rle as RL
    from bonai_amd.scene import SceneDetector
    H, W, t = 384, 320, 256
    scene = _scene_u8(H, W, 22).cuda()
    det = SceneDetector(model, tile=t, overlap=128)
    res = det.run(scene)
    origins = [[0, 0], [64, 0], [0, 128], [64, 128]]
    assert res.origins.tolist() == origins
    boxes, scores, logits, offsets, tiles = [], [], [], [], []
    for k, (x0, y0) in enumerate(origins):                               # the four tiles, cut and run here
        img = K.image_prep_d4(scene[y0:y0 + t, x0:x0 + t][None].contiguous(), [0], [False], MEAN, STD)
        with torch.no_grad():
            x = model.extract_feat(img)
            metas = [_meta(t, t)]
            d, l, m, o = model.roi_head.simple_test_device(x, model.rpn_head.simple_test_rpn(x, metas), metas)
        assert d.is_cuda and m.is_cuda and o.is_cuda and (d.shape[0] == 0 or m.shape[1:] == (28, 28))
        if d.shape[0]:
            boxes.append(d[:, :4].cpu().numpy()), scores.append(d[:, 4].cpu().numpy()), logits.append(m), offsets.append(o.cpu().numpy())
            tiles.append(np.full(d.shape[0], k, np.int32))
    boxes, scores, tiles, offsets = np.concatenate(boxes), np.concatenate(scores), np.concatenate(tiles), np.concatenate(offsets)
    logits = torch.cat(logits)
    thr = model.roi_head.test_cfg.mask_thr_binary
    scene_boxes = R.translate(boxes, tiles, origins)
    bitmaps = K.mask_paste(logits, torch.from_numpy(scene_boxes).cuda(), H, W, thr)
    keep = R.merge(bitmaps.bool().cpu().numpy(), scene_boxes, boxes, tiles, scores, origins, (t, t), H, W, 0.5, 2)
    print(f'four tiles: {len(keep)} detections, {int(keep.sum())} kept, per tile {np.bincount(tiles, minlength=4).tolist()}')
    assert len(set(tiles.tolist())) > 1 and 0 < keep.sum()
    assert np.array_equal(res.bboxes, np.concatenate([scene_boxes, scores[:, None]], 1)[keep])
    assert np.array_equal(res.tiles, tiles[keep]) and np.array_equal(res.offsets, offsets[keep])
    want = RL.rle_encode_masks(bitmaps[torch.from_numpy(keep).cuda()])
    assert len(res.roofs) == len(want) and all(a == b for a, b in zip(res.roofs, want)) and res.footprints is None
    assert want[0]['size'] == [H, W]


def test_refusals(model):
    from bonai_amd.scene import SceneDetector
    with pytest.raises(ValueError, match='8192'):
        SceneDetector(model, tile=256, overlap=128).run(torch.zeros(32, 8200, 3, dtype=torch.uint8, device='cuda'))
    pipeline = [dict(type='MultiScaleFlipAug', img_scale=(256, 256), flip=True, transforms=[])]
    with pytest.raises(ValueError, match='test-time augmentation'):
        SceneDetector(model, tile=256, overlap=128, cfg=dict(data=dict(test=dict(pipeline=pipeline, img_scale=(256, 256)))))
    assert SceneDetector(model, cfg=dict(data=dict(test=dict(img_scale=(1024, 512))))).tile == (512, 1024)     # img_scale is (w, h)
    cfg = model.roi_head.test_cfg
    cfg['paste_min_score'] = 0.4
    try:
        with pytest.raises(ValueError, match='paste_min_score'):
            SceneDetector(model, tile=256, overlap=128)
    finally:
        cfg.pop('paste_min_score')
    with pytest.raises(ValueError, match='multiples of 32'):
        SceneDetector(model, tile=250, overlap=128)
    with pytest.raises(ValueError):
        SceneDetector(model, tile=256, overlap=256)
