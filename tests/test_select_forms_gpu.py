"""GPU: every kernel form of csrc/nms.hip (segmented NMS mask + scan, radix sort, radix-select / bitonic top-k in one and two stages,
rank merge of sorted runs, soft-NMS) and boxes.hip's rpn_finalize against the references of tests/test_select_forms_cpu.py, which owns
the inputs, the references and the census of which path each case reaches.  Every comparison is exact (keys as bit patterns, so that
-0.0 for +0.0 would fail) except the gaussian soft-NMS scores, which are held to a derived bound (test_select_forms_cpu.gauss_bound)."""
import numpy as np
import pytest
import torch

from bonai_amd import kernels as K
from bonai_amd import lib as L

from test_select_forms_cpu import (FIN_POST, FIN_STRIDE, FIN_VALID, LEVELS, NMS_FAMILIES, NMS_SIZES, NMS_THR, PREDICATES, SNMS_MIN,
                                   SNMS_SIGMA, SNMS_SIZES, SNMS_THR, SORT_SEGMENTS, SORT_SIZES, TOPK_K, TOPK_KEYSETS,
                                   TWO_STAGE_KEYSETS, TWO_STAGE_LENS, TWO_STAGE_MAX_SEGMENT, TWO_STAGE_RUNS, F, finalize_case,
                                   finalize_reference, gaussian_case, gaussian_ratio, gaussian_reference, head_index, levels_reference,
                                   masked_keys, nms_boxes, nms_code, nms_levels_case, nms_multi_case, nms_reference, oracle_keep,
                                   snms_case, sort_case, sort_reference, topk_code, topk_keys, topk_layout, two_stage_keys,
                                   two_stage_layout)
from oracle import cops

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.view(torch.int32)


def assert_heads(got_k, got_v, ref_bits, ref_vals, head, what):
    """Keys (bit patterns) and values equal on the head positions; nothing is said about the unwritten rest."""
    h = dev(head)
    assert torch.equal(bits(got_k)[h], dev(ref_bits.view(np.int32))[h]), what
    assert torch.equal(got_v.long()[h], dev(ref_vals)[h]), what


# ---- 1. top-k, one stage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TOPK_KEYSETS)
def test_topk_one_stage(name):
    """Segments at every start residue mod 4 (the 16-byte body, its four-in-flight loop and its scalar tail where the start is aligned;
    the scalar walk elsewhere), every k: plain, with explicit values, and with the key mask at every residue of the MASK's address."""
    keys, mask, values = topk_keys(name)
    off = topk_layout()
    n, longest = len(keys), int(np.diff(off).max())
    assert longest <= K.TOPK_MAX_SEGMENT
    dk, doff, dvals = dev(keys), dev(off), dev(values)
    ref_b, ref_i = sort_reference(keys, off)
    _, ref_v = sort_reference(keys, off, values)
    mkeys = masked_keys(keys, mask)
    mref_b, mref_i = sort_reference(mkeys, off)
    _, mref_v = sort_reference(mkeys, off, values)
    dmk = dev(mkeys)
    big = torch.zeros(n + 8, dtype=torch.uint8, device='cuda')
    for k in TOPK_K:
        head = head_index(off, k)
        gk, gv = K.segmented_topk_desc(dk, doff, k, max_segment=longest)
        assert_heads(gk, gv, ref_b, ref_i, head, (name, k))
        gk, gv = K.segmented_topk_desc(dk, doff, k, values=dvals, max_segment=longest)
        assert_heads(gk, gv, ref_b, ref_v, head, (name, k, 'values'))
        wk, wv = K.segmented_topk_desc(dmk, doff, k, max_segment=longest)               # where(mask, key, -1) through the plain form
        assert_heads(wk, wv, mref_b, mref_i, head, (name, k, 'where'))
        for mo in range(4):
            big.zero_()
            view = big[mo:mo + n]
            view.copy_(dev(mask))
            assert view.data_ptr() % 4 == mo
            mk_, mv_ = K.segmented_topk_desc(dk, doff, k, max_segment=longest, key_mask=view)
            assert_heads(mk_, mv_, mref_b, mref_i, head, (name, k, 'mask at', mo))
            h = dev(head)
            assert torch.equal(bits(mk_)[h], bits(wk)[h]) and torch.equal(mv_[h], wv[h])
        both_k, both_v = K.segmented_topk_desc(dk, doff, k, values=dvals, max_segment=longest, key_mask=dev(mask))   # values AND mask
        assert_heads(both_k, both_v, mref_b, mref_v, head, (name, k, 'values and mask'))
    bk, bv = K.segmented_topk_desc(dk, doff, 1000, max_segment=longest, key_mask=dev(mask).bool())          # a bool mask
    assert_heads(bk, bv, mref_b, mref_i, head_index(off, 1000), (name, 'bool mask'))


def test_topk_k_outside_the_range():
    keys, _, _ = topk_keys('heavy_ties')
    off = topk_layout()
    dk, doff = dev(keys), dev(off)
    assert topk_code(0) == 1 and topk_code(4097) == 1
    with pytest.raises(L.LoftHipError):
        K.segmented_topk_desc(dk, doff, 0, max_segment=int(np.diff(off).max()))
    fk, fv = K.segmented_topk_desc(dk, doff, 4097, max_segment=int(np.diff(off).max()))    # the full sort
    ref_b, ref_i = sort_reference(keys, off)
    assert torch.equal(bits(fk), dev(ref_b.view(np.int32))) and torch.equal(fv.long(), dev(ref_i))


# ---- 2. top-k, two stages ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('runs', TWO_STAGE_RUNS)
def test_topk_two_stages_at_small_shapes(runs, monkeypatch):
    """TOPK_MAX_SEGMENT = 2048 sends these segments through sub-range top-k + rank merge; 13 and 25 runs per longest segment reach the
    merge's second and third lock-step group of 12 runs.  Equal to the one-stage kernel and to the reference."""
    off = two_stage_layout()
    lens, longest = list(TWO_STAGE_LENS), max(TWO_STAGE_LENS)
    doff = dev(off)
    # K._TOPK_TABLES is keyed by (lengths, k, device) only -- not by TOPK_RUNS or TOPK_MAX_SEGMENT, which are constants outside this
    # test.  Tables built here for one run count must therefore not outlive this parametrisation: the `finally` drops them, and the
    # run_count assertion below fails if tables of another run count were ever served.
    before = set(K._TOPK_TABLES)
    try:
        for name in TWO_STAGE_KEYSETS:
            keys = two_stage_keys(name)
            dk = dev(keys)
            ref_b, ref_i = sort_reference(keys, off)
            for k in TOPK_K:
                head = head_index(off, k)
                one_k, one_v = K.segmented_topk_desc(dk, doff, k, max_segment=longest)
                assert_heads(one_k, one_v, ref_b, ref_i, head, (name, k, 'one stage'))
                with monkeypatch.context() as m:
                    m.setattr(K, 'TOPK_MAX_SEGMENT', TWO_STAGE_MAX_SEGMENT)
                    m.setattr(K, 'TOPK_RUNS', runs)
                    tabs = K._topk_two_stage_tables(lens, k, dk.device)
                    assert tabs is not None and max(tabs['run_count'].tolist()) == runs
                    two_k, two_v = K.segmented_topk_desc(dk, doff, k, max_segment=longest, seg_lengths=lens)
                assert_heads(two_k, two_v, ref_b, ref_i, head, (name, k, runs))
                h = dev(head)
                assert torch.equal(bits(two_k)[h], bits(one_k)[h]) and torch.equal(two_v[h], one_v[h])
    finally:
        for key in set(K._TOPK_TABLES) - before:
            del K._TOPK_TABLES[key]
    assert set(K._TOPK_TABLES) == before and K.TOPK_MAX_SEGMENT == 32768 and K.TOPK_RUNS == 10


# ---- 3. radix sort -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nseg', SORT_SEGMENTS)
def test_radix_sort(nseg):
    """9, 9, 10, 11 and 12 passes (the value ping-pong ends in vals_out for odd AND even pass counts); one item to 133 121 (a scan
    table longer than the scan's workgroup); with the default values and with explicit ones; with the last segment empty and with keys
    in it (the last pass of 17 and 4097 segments sorts on that segment's bit alone)."""
    for n, tail in [(n, t) for n in SORT_SIZES for t in ((False, True) if nseg >= 17 else (False,))]:
        keys, off, values = sort_case(n, nseg, tail)
        ref_b, ref_i = sort_reference(keys, off)
        _, ref_v = sort_reference(keys, off, values)
        gk, gv = K.segmented_sort_desc(dev(keys), dev(off))
        assert torch.equal(bits(gk), dev(ref_b.view(np.int32))), (n, nseg)
        assert torch.equal(gv.long(), dev(ref_i)), (n, nseg)
        gk, gv = K.segmented_sort_desc(dev(keys), dev(off), dev(values))
        assert torch.equal(bits(gk), dev(ref_b.view(np.int32))), (n, nseg, 'values')
        assert torch.equal(gv.long(), dev(ref_v)), (n, nseg, 'values')


# ---- 4. NMS --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', NMS_SIZES)
@pytest.mark.parametrize('family', NMS_FAMILIES)
def test_nms_single_segment(family, n):
    boxes = nms_boxes(family, n)
    db, off = dev(boxes), torch.tensor([0, n], dtype=torch.int64, device='cuda')
    for pred in PREDICATES:
        want = dev(nms_reference(family, n, pred).astype(np.uint8))
        got = K.nms_segmented(db, off, NMS_THR, max_segment=n, predicate=pred)
        assert torch.equal(got, want), (family, n, pred)
        assert torch.equal(K.nms_segmented(db, off, NMS_THR, max_segment=n, predicate=pred, covered=True), want)
        assert torch.equal(K.nms_segmented(db, off, NMS_THR, predicate=pred), want)          # max_segment read from the offsets


@pytest.mark.parametrize('empty_at', [0, 5, 10])
def test_nms_many_segments_in_one_launch(empty_at):
    """Segments of 1 to 8256 boxes in varying order: the row stride of the tile matrix is the longest segment's, the tile rows of
    neighbours abut, the ONE and the wide scan run side by side; per-segment shifts up to the edge of the exact integers."""
    boxes, off, shift, segs = nms_multi_case(empty_at)
    db, doff = dev(boxes), dev(off)
    for pred in PREDICATES:
        want = np.concatenate([nms_reference(f, n, pred) if n else np.zeros(0, dtype=bool) for f, n, _ in segs])
        shifted = np.concatenate([oracle_keep(boxes[a:b], NMS_THR, pred, s) if (b > a and s) else want[a:b]
                                  for (f, n, s), a, b in zip(segs, off[:-1], off[1:])])
        assert np.array_equal(want, shifted)
        want = dev(want.astype(np.uint8))
        got = K.nms_segmented(db, doff, NMS_THR, seg_shift=dev(shift), max_segment=int(np.diff(off).max()), predicate=pred)
        assert torch.equal(got, want), pred
        assert torch.equal(K.nms_segmented(db, doff, NMS_THR, max_segment=int(np.diff(off).max()), predicate=pred, covered=True), want)
        # a loose bound on the longest segment changes the layout of the tile matrix, not the flags
        assert torch.equal(K.nms_segmented(db, doff, NMS_THR, seg_shift=dev(shift), max_segment=8256 + 640, predicate=pred), want)


def test_nms_level_shift_on_the_device_equals_the_given_shift():
    boxes, off, img_max, shift, ids, img = nms_levels_case()
    db, doff = dev(boxes), dev(off)
    longest = int(np.diff(off).max())
    for pred in PREDICATES:
        want = dev(levels_reference(pred).astype(np.uint8))
        a = K.nms_segmented(db, doff, NMS_THR, seg_shift=dev(shift), max_segment=longest, predicate=pred)
        for covered in (False, True):
            b = K.nms_segmented(db, doff, NMS_THR, max_segment=longest, predicate=pred, img_max=dev(img_max), levels=LEVELS,
                                covered=covered)
            assert torch.equal(a, b), (pred, covered)
        assert torch.equal(a, want), pred
        assert torch.equal(a[int(off[0]):int(off[0]) + 64], a[int(off[2]):int(off[2]) + 64])     # one list in two levels: no cross-talk


def test_nms_refusals_launch_nothing():
    assert nms_code(max_segment=32769) == 1 and nms_code(predicate=2) == 1 and nms_code(levels=4, S=6) == 1
    assert nms_code(max_segment=32769, levels=2, S=6) == 1
    assert nms_code() == 0 and nms_code(levels=3, S=6) == 0                                  # the same calls, accepted
    db, off = torch.zeros(128, 4, device='cuda'), torch.tensor([0, 64, 128], dtype=torch.int64, device='cuda')
    with pytest.raises(L.LoftHipError):
        K.nms_segmented(db, off, NMS_THR, max_segment=32769)
    with pytest.raises(L.LoftHipError):
        K.nms_segmented(db, off, NMS_THR, max_segment=64, img_max=torch.zeros(2, device='cuda'), levels=4)
    with pytest.raises(KeyError):
        K.nms_segmented(db, off, NMS_THR, max_segment=64, predicate='host')


# ---- 5. rpn_finalize -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('post', FIN_POST)
def test_rpn_finalize(post):
    scores, idx, boxes = finalize_case()
    props, counts = K.rpn_finalize(dev(scores), dev(idx), dev(boxes), len(FIN_VALID), FIN_STRIDE, post)
    want_p, want_c = finalize_reference(scores, idx, boxes, post)
    assert torch.equal(bits(props), dev(want_p.view(np.int32))) and torch.equal(counts, dev(want_c))
    assert counts.tolist() == [min(v, post) for v in FIN_VALID]


# ---- 6. soft-NMS ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ties', [False, True], ids=['distinct', 'ties'])
@pytest.mark.parametrize('method', ['naive', 'linear'])
@pytest.mark.parametrize('n', SNMS_SIZES)
def test_soft_nms_bit_equal(n, method, ties):
    """ties: equal scores, where the first POSITION wins -- the arrangement the hole / fill compaction leaves decides the result."""
    boxes, scores = snms_case(n, ties=ties)
    dref, iref = cops.soft_nms(torch.from_numpy(boxes), torch.from_numpy(scores), SNMS_THR, SNMS_SIGMA, SNMS_MIN, method)
    d, i = K.soft_nms(dev(boxes), dev(scores), SNMS_THR, SNMS_SIGMA, SNMS_MIN, method)
    assert i.shape == iref.shape and torch.equal(i.cpu(), iref)
    assert torch.equal(bits(d.cpu()), bits(dref))


@pytest.mark.parametrize('n', SNMS_SIZES)
def test_soft_nms_gaussian_within_the_derived_bound(n):
    """The float64 trajectory of these inputs is decided (no winner within the bounds of its runner-up, no score within its bound of
    min_score: asserted on the CPU), so the index list must be the reference's; every score within gauss_bound of the float64 one."""
    boxes, scores = gaussian_case(n)
    ref = gaussian_reference(n)
    d, i = K.soft_nms(dev(boxes), dev(scores), SNMS_THR, SNMS_SIGMA, SNMS_MIN, 'gaussian')
    assert i.shape[0] == len(ref['inds']) and np.array_equal(i.cpu().numpy(), ref['inds'])
    assert np.array_equal(d.cpu().numpy()[:, :4], ref['dets'][:, :4].astype(F))
    ratio = gaussian_ratio(d.cpu().numpy(), i.cpu().numpy(), ref)
    print(f'gaussian n={n}: kernel max |got - ref| / bound = {ratio:.3f}, most decays {ref["decays"].max()}')
    assert ratio <= 1.0
