"""GPU: loft_iou_assign and loft_random_sample (csrc/boxes.hip) against the numpy references of tests/assign_sample_restatement.py,
which owns the inputs, the references and the censuses of which path each case reaches (tests/test_assign_sample_cpu.py asserts
them).  Every comparison is exact: indices, validity bytes and the bit patterns of the overlaps.  One test per kernel and kind runs
all its rows and names every row that missed."""
import numpy as np
import pytest
import torch

from bonai_amd import kernels as K
from bonai_amd import lib as L

import assign_sample_restatement as R

pytestmark = pytest.mark.gpu

MODES = {'first': 0, 'random': 1}
IDX_SENTINEL, VALID_SENTINEL = -7, 0xCC


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_sampler(gt_inds, num, max_pos, mode, seed):
    """The C entry point with an explicit seed.  Outputs are prefilled with sentinels and have one guard row beyond B."""
    lib = L.load()
    B, N = gt_inds.shape
    P, Q = min(max_pos, N), min(num, N)
    g = dev(gt_inds)
    out = [torch.full((B + 1, P), IDX_SENTINEL, dtype=torch.int64, device='cuda'),
           torch.full((B + 1, P), VALID_SENTINEL, dtype=torch.uint8, device='cuda'),
           torch.full((B + 1, Q), IDX_SENTINEL, dtype=torch.int64, device='cuda'),
           torch.full((B + 1, Q), VALID_SENTINEL, dtype=torch.uint8, device='cuda')]
    ws = torch.empty(int(lib.loft_random_sample_workspace_bytes(B, N)), dtype=torch.uint8, device='cuda')
    L.check(lib.loft_random_sample(L.ptr(g), B, N, num, max_pos, MODES[mode], seed, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]),
                                   L.ptr(out[3]), L.ptr(ws), L.stream()), 'loft_random_sample')
    return [o.cpu().numpy() for o in out]


def sampler_misses(got, ref, B):
    """Names of the outputs that differ anywhere in [0, B) x capacity, or whose guard row was written."""
    bad = []
    for name, o, r in zip(('pos_idx', 'pos_valid', 'neg_idx', 'neg_valid'), got, ref):
        if not np.array_equal(o[:B], r):
            rows = sorted(set(np.nonzero(o[:B] != r)[0].tolist()))
            bad.append(f'{name} images {rows}')
        sentinel = IDX_SENTINEL if o.dtype == np.int64 else VALID_SENTINEL
        if not (o[B] == sentinel).all():
            bad.append(f'{name} guard row written')
        if o.dtype == np.uint8 and not np.isin(o[:B], (0, 1)).all():
            bad.append(f'{name} not 0 / 1')
    return bad


def test_sampler_exact():
    """Every row of the case table, all four outputs over the whole capacity; the twins (two images with the same gt_inds) draw
    differently, each as the reference says."""
    missed = {}
    for name, (g, num, max_pos, mode, seed) in R.SAMPLER_CASES().items():
        got = run_sampler(g, num, max_pos, mode, seed)
        bad = sampler_misses(got, R.sample_reference(g, num, max_pos, mode, seed), g.shape[0])
        if name in R.TWINS and (np.array_equal(got[0][0], got[0][1]) or np.array_equal(got[2][0], got[2][1])):
            bad.append('two images drew the same subset')
        if bad:
            missed[name] = bad
    assert not missed, missed


def test_sampler_ties():
    """The k-th and (k+1)-th smallest keys are equal (committed seeds: pooled, pre-filter, overflow and full-passes paths).  k - 1
    takes neither of the pair, k the one with the lower index, k + 1 both."""
    missed = {}
    for name, spec in R.TIE_SPECS.items():
        _, k = R.TIE_SEEDS[name]
        lo, hi = R.tie_pair(name)
        c = spec['cls']
        for kk, want in ((k - 1, (False, False)), (k, (True, False)), (k + 1, (True, True))):
            case = R.tie_case(name, kk)
            got = run_sampler(*case)
            bad = sampler_misses(got, R.sample_reference(*case), 1)
            took = got[2 * c][0][got[2 * c + 1][0] == 1]
            if (lo in took, hi in took) != want:
                bad.append(f'pair ({lo}, {hi}) taken as {(lo in took, hi in took)}')
            if bad:
                missed[(name, kk)] = bad
    assert not missed, missed


def rng_state():
    return torch.initial_seed(), torch.get_rng_state(), torch.cuda.get_rng_state()


def restore_rng(state):
    torch.manual_seed(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2])


def test_sampler_seed_derivation():
    """K.random_sample: seed = initial_seed * 6364136223846793005 + calls * 1442695040888963407 mod 2^64 with the counter advanced
    before the draw, by one per call."""
    g, num, max_pos, _, _ = R.SAMPLER_CASES()['pooled_N3080_rcnn']
    dg = dev(g)
    calls, state = K._SAMPLE_CALLS[0], rng_state()
    try:
        torch.manual_seed(20240229)
        K._SAMPLE_CALLS[0] = 41
        for n in (42, 43):
            got = K.random_sample(dg, num, max_pos)
            assert K._SAMPLE_CALLS[0] == n
            seed = (20240229 * 6364136223846793005 + n * 1442695040888963407) % 2 ** 64
            ref = R.sample_reference(g, num, max_pos, 'random', seed)
            for o, r in zip(got, ref):
                assert np.array_equal(o.cpu().numpy().astype(r.dtype), r), n
        first = K.random_sample(dg, num, max_pos, mode='first')
        assert K._SAMPLE_CALLS[0] == 44
        for o, r in zip(first, R.sample_reference(g, num, max_pos, 'first', 0)):
            assert np.array_equal(o.cpu().numpy().astype(r.dtype), r)
    finally:
        K._SAMPLE_CALLS[0] = calls
        restore_rng(state)


def run_assigner(sc, thr, lq):
    gi, mo = K.iou_assign(dev(sc['boxes']), dev(sc['nbox']), dev(sc['gts']), dev(sc['ngt']), thr[0], thr[1], thr[2], lq)
    return gi.cpu().numpy(), mo.cpu().numpy()


def test_assigner_exact():
    """Every scene under every form: gt_inds over [0, Nmax) with -1 at and beyond nbox, max_ov bit for bit over [0, nbox) (beyond
    nbox it is not written; no caller reads it)."""
    missed = {}
    for name, sc in R.ASSIGNER_SCENES().items():
        for thr, lq in R.FORMS:
            gi, mo = run_assigner(sc, thr, lq)
            ref_gi, ref_mo = R.scene_reference(sc, thr, lq)
            bad = []
            if not np.array_equal(gi, ref_gi):
                bad.append('gt_inds images %s' % sorted(set(np.nonzero(gi != ref_gi)[0].tolist())))
            for b, r in enumerate(ref_mo):
                if not np.array_equal(mo[b, :r.shape[0]].view(np.int32), r.view(np.int32)):
                    bad.append(f'max_ov image {b}')
            if bad:
                missed[(name, thr, lq)] = bad
    assert not missed, missed


CHAIN_ROWS = (('size_N1030_K80', (0.7, 0.3, 0.3), True, 256, 128), ('anchors', (0.5, 0.5, 0.0), True, 64, 16),
              ('geometry', (0.5, 0.25, 0.25), False, 32, 8))


def test_assigner_into_sampler():
    """The device assigner's gt_inds (ragged B = 3) straight into the device sampler in mode random: reference of the reference."""
    missed = {}
    calls, state = K._SAMPLE_CALLS[0], rng_state()
    try:
        torch.manual_seed(7)
        for name, thr, lq, num, max_pos in CHAIN_ROWS:
            sc = R.ASSIGNER_SCENES()[name]
            gi, _ = K.iou_assign(dev(sc['boxes']), dev(sc['nbox']), dev(sc['gts']), dev(sc['ngt']), thr[0], thr[1], thr[2], lq)
            got = K.random_sample(gi, num, max_pos)
            seed = (7 * 6364136223846793005 + K._SAMPLE_CALLS[0] * 1442695040888963407) % 2 ** 64
            ref_gi, _ = R.scene_reference(sc, thr, lq)
            ref = R.sample_reference(ref_gi, num, max_pos, 'random', seed)
            bad = [n for n, o, r in zip(('pos_idx', 'pos_valid', 'neg_idx', 'neg_valid'), got, ref)
                   if not np.array_equal(o.cpu().numpy().astype(r.dtype), r)]
            draws = [r['draws'] for r in R.sample_census(ref_gi, num, max_pos, 'random', seed)]
            if sum(draws) < 3:
                bad.append('the row draws no strict subsets')
            if bad:
                missed[name] = bad
    finally:
        K._SAMPLE_CALLS[0] = calls
        restore_rng(state)
    assert not missed, missed
