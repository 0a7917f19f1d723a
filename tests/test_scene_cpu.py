"""CPU: the tile grid of bonai_amd/scene.py against answers derived by hand, and the greedy loop of tests/scene_restatement.py --
the statement the GPU tests hold loft_scene_suppress to -- pinned with hand-derived cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_restatement as R  # noqa: E402

from bonai_amd.scene import SceneResult, tile_grid  # noqa: E402


def _grid(H, W, tile, overlap):
    g = tile_grid(H, W, tile, overlap)
    assert g.dtype == np.int32 and g.ndim == 2 and g.shape[1] == 2
    return g.tolist()


def test_tile_grid_hand_cases():
    assert _grid(50, 64, 64, 32) == [[0, 0]]                                   # L <= t on both axes: one padded tile
    assert _grid(64, 65, 64, 32) == [[0, 0], [1, 0]]                           # L = t + 1: ceil(33 / 32) = 2 tiles, the last at L - t = 1
    # H = 96: ceil(64 / 32) = 2 -> 0, 32; W = 80: ceil(48 / 32) = 2 -> 0, 16; row-major, (x0, y0)
    assert _grid(96, 80, (64, 64), 32) == [[0, 0], [16, 0], [0, 32], [16, 32]]
    # L = 100: ceil(68 / 32) = 3 -> 0, 32 and the last at 36, not 64: it shares 32 + 64 - 36 = 60 > 32 pixels with its neighbour
    assert _grid(64, 100, 64, 32) == [[0, 0], [32, 0], [36, 0]]
    assert _grid(97, 130, 64, 32) == [[x, y] for y in (0, 32, 33) for x in (0, 32, 64, 66)]
    assert _grid(40, 100, (32, 64), 0) == [[0, 0], [36, 0], [0, 8], [36, 8]]   # tile = (th, tw), no overlap asked for
    assert _grid(384, 320, 256, 128) == [[0, 0], [64, 0], [0, 128], [64, 128]]


@pytest.mark.parametrize('t, overlap', [(64, 32), (64, 0), (32, 31), (48, 16), (7, 3)])
def test_tile_grid_covers_every_pixel_with_the_overlap(t, overlap):
    for L in range(1, 4 * t + 3):
        xs = [x for x, _ in _grid(t, L, t, overlap)]
        assert xs == sorted(set(xs)) and xs[0] == 0
        if L <= t:
            assert xs == [0]
            continue
        assert xs[-1] + t == L                                                # the last tile ends at the scene's edge, unpadded
        covered = np.zeros(L, bool)
        for x in xs:
            covered[x:x + t] = True
        assert covered.all()
        assert all(a + t - b >= overlap for a, b in zip(xs, xs[1:])), (L, xs)
        assert len(xs) == -(-(L - overlap) // (t - overlap))


def test_tile_grid_refusals():
    for bad in (dict(H=64, W=64, tile=64, overlap=64), dict(H=64, W=64, tile=(64, 32), overlap=32), dict(H=0, W=64, tile=64, overlap=0),
                dict(H=64, W=-3, tile=64, overlap=0), dict(H=64, W=64, tile=0, overlap=0), dict(H=64, W=64, tile=64, overlap=-1),
                dict(H=64.0, W=64, tile=64, overlap=0), dict(H=64, W=64, tile=64.5, overlap=0), dict(H=64, W=64, tile=64, overlap=1.5),
                dict(H=True, W=64, tile=64, overlap=0)):
        with pytest.raises(ValueError):
            tile_grid(bad['H'], bad['W'], bad['tile'], bad['overlap'])


def _keep(records, area, scores, trunc=None, thr=0.5):
    return R.greedy(records, area, scores, trunc if trunc is not None else [False] * len(area), thr).astype(int).tolist()


# (records, area, scores, truncated, merge_thr) -> keep; shared with tests/test_scene_gpu.py, where the device runs them
GREEDY_CASES = {
    # a > b > c, edges a-b and b-c: b falls to a, so nothing kept is a neighbour of c ("any better neighbour" would drop c too)
    'chain': ([(0, 1, 80), (1, 2, 80)], [100, 100, 100], [.9, .8, .7], [0, 0, 0], .5, [1, 0, 1]),
    'truncated_high_score_loses': ([(0, 1, 60)], [100, 100], [.9, .3], [1, 0], .5, [0, 1]),
    'equal_scores_lower_index_wins': ([(0, 1, 60)], [100, 100], [.5, .5], [0, 0], .5, [1, 0]),
    'both_truncated_score_decides': ([(0, 1, 60)], [100, 100], [.4, .6], [1, 1], .5, [0, 1]),
    'area_zero_has_no_edge': ([(0, 1, 0), (1, 2, 5)], [0, 100, 0], [.9, .8, .7], [0, 0, 0], .0, [1, 1, 1]),
    'inter_equal_to_the_bound_is_no_edge': ([(0, 1, 40)], [100, 80], [.9, .8], [0, 0], .5, [1, 1]),     # 40 == 0.5 * min(100, 80)
    'inter_one_above_the_bound': ([(0, 1, 41)], [100, 80], [.9, .8], [0, 0], .5, [1, 0]),
    'record_order_reversed_chain': ([(2, 3, 90), (1, 2, 90), (0, 1, 90)], [100] * 4, [.9, .8, .7, .6], [0] * 4, .5, [1, 0, 1, 0]),
    'no_records': ([], [10, 0, 30], [.1, .2, .3], [1, 0, 1], .5, [1, 1, 1]),
}


@pytest.mark.parametrize('name', sorted(GREEDY_CASES))
def test_restatement_greedy_hand_cases(name):
    recs, area, scores, trunc, thr, want = GREEDY_CASES[name]
    assert _keep(recs, area, scores, trunc, thr) == want
    assert _keep({(i, j): c for i, j, c in recs}, area, scores, trunc, thr) == want


def test_restatement_pair_counts_and_truncation():
    bm = np.zeros((3, 8, 12), bool)
    bm[0, 2:6, 1:5] = True
    bm[1, 3:7, 3:8] = True
    bm[2, 2:6, 1:5] = True
    boxes = np.array([[2, 3, 4, 5], [4, 4, 7, 6], [2, 3, 4, 5]], np.float32)
    area, recs = R.pair_counts(bm, boxes, [0, 1, 0])
    assert area.tolist() == [16, 20, 16] and recs == {(0, 1): 6, (1, 2): 6}             # (0, 2): the same tile, no record
    assert R.windows(boxes, 8, 12).tolist() == [[1, 5, 2, 6], [3, 8, 3, 7], [1, 5, 2, 6]]
    assert R.windows([[10, 10, 20, 20], [22, 22, 30, 30]], 97, 130).tolist() == [[9, 21, 9, 21], [21, 31, 21, 31]]
    assert not R.windows_meet([9, 21, 9, 21], [21, 31, 21, 31])                           # they touch at a corner only
    origins = [[0, 0], [32, 0]]
    tb = np.array([[1, 1, 20, 20], [1.5, 5, 20, 20], [30, 5, 62.5, 20], [30, 5, 61, 20], [5, 1, 20, 63]], np.float32)
    # tile 0 at x = 0: its left edge is the scene's; its right edge (x = 64 of 96) is not.  Tile 1 at x = 32 ends at the scene's edge.
    assert R.truncated(tb, [0, 1, 0, 0, 1], origins, (64, 64), 64, 96, 2).tolist() == [False, True, True, False, False]
    assert R.translate(tb[:2], [0, 1], origins).tolist() == [[1, 1, 20, 20], [33.5, 5, 52, 20]]


def test_scene_result_tuple_layout():
    z = np.zeros
    empty = SceneResult((8, 8), 1, z((1, 2), np.int32), z((0, 5), np.float32), z((0,), np.int64), z((0, 2), np.float32), z((0,), np.int32),
                        [], None).as_result_tuple()
    assert len(empty) == 3 and empty[0][0].shape == (0, 5) and empty[1] == [[]] and empty[2] == [[], []]
    r = SceneResult((8, 8), 2, z((1, 2), np.int32), np.arange(15, dtype=np.float32).reshape(3, 5), np.array([1, 0, 1]),
                    np.ones((3, 2), np.float32), z((3,), np.int32), ['a', 'b', 'c'], ['A', 'B', 'C']).as_result_tuple()
    assert len(r) == 4 and r[0][0].tolist() == [[5, 6, 7, 8, 9]] and r[0][1].shape == (2, 5)
    assert r[1] == [['b'], ['a', 'c']] and r[3] == [['B'], ['A', 'C']] and r[2].shape == (3, 2)
