"""GPU: every forward and backward kernel form of RoIAlign (csrc/roi_align.hip) against the defining sums in float64, on the built
lists of tests/test_roi_forms_cpu.py (FORMS / BWD_FORMS x lists; the census of the lists and the reference-versus-oracle check run there,
without a GPU).  Every entry point writes into buffers pre-filled with NaN: an element a kernel does not write fails the comparison.

  (A) lattice operands (lists L7 / L14 / crowd / one16: starts on the quarter-pixel lattice, bins in {1/4 .. 8}, integer features and
      gradients of magnitude <= 4): every weight, product and partial sum is a short dyadic number (grain_ok proves it per case from the
      reference and the list's tables: all terms are multiples of list_grain and sum|terms| < 2^24 grains), so fp32 outputs must EQUAL
      the reference and 16-bit outputs the reference rounded once to nearest-even -- in write mode and in accumulate mode (old 16-bit
      value + exact sum, rounded once), sorted and unsorted, for the VALU, MFMA and pipelined backward and the multi-list route.  No tolerance.
  (B) random operands (rounded to the operand type first) on RoIs off the lattice (R7 / R14): per element
          |got - ref| <= (n + c) u mag + u16 |ref|,     u = 2^-24,
      mag = the same sum over absolute values, n = the terms of the element's sum, c = the roundings of one term, from the code:
        * hat weight of a sample: l = v - floor(v) exact, h = 1 - l one rounding.
        * sample-order forms (roi_align_fwd_kernel, roi_sample_bins, the LDS form): w = hy hx: 2 + 1; w v: 1 (the LDS form's fma rounds
          it with the addition); the mean: 1 (division) or reciprocal-then-multiply 2.  c = 3 + 1 + 2 = 6; n = 4 per valid sample.
        * separable walks: WY[p][y] is a sum of <= grid_h positive hat weights, each rounded once and passed through <= grid_h - 1
          additions: grid_h u relative; WX likewise; wy v and colsum wx: one each in the 8-byte kernel (no contraction), none in the
          16-byte kernel's fmas; 1 / count and the product: 2.  c = grid_h + grid_w + 4; the pixel terms of a bin (rows x columns
          with weight) number at most the (sample, corner) terms n, half-wave partial sums included.
        * VALU backward: WY, WX as above; inv = 1 / count 1, WY inv 1, (wy inv) wx 1, x gout 1; the rotation sum of gout n_rot - 1.
          c = grid_h + grid_w + 4 + (n_rot - 1), with the list's largest grid; n = the (RoI, bin, rotation) terms landing on the pixel.
        * MFMA backward (and its pipelined twin): a = (WY inv) WX: 3 + grid_h + grid_w; a is split into two 16-bit pieces, hi + lo =
          a to 2^-16 relative as the kernel's comment claims: + 2^-16 mag; the products of 16-bit values are exact in fp32, every term
          is two addends: 2 n additions.  For n_rot = 4 the staging sums the four rotations in fp32 and ROUNDS THE SUM TO 16 BITS
          before the product (f32_to_bf16(sacc) in the gout staging loop): + u16 mag.
      16-bit outputs add one rounding of that type: u16 (|ref| + bound), u16 = half an ulp (2^-8 bfloat16; 2^-11 binary16 + half its
      subnormal step 2^-25).  No element is left out.
  (C) dispatch: ROI_AUTO without tuning bits == per RoI row, bit for bit, the form K.roi_fwd_form says the RoI resolves to (rows of
      LDS RoIs against a launch where everything that can stage does, rows of walk / loop RoIs against a launch with staging off);
      nsplit 1 == 2 == 3; ordered == unordered; roi_align_bwd_multi with one list == roi_align_bwd."""
import functools

import numpy as np
import pytest
import torch

from test_roi_forms_cpu import (B, BWD_FORMS, BWD_IDS, FORMS, FORM_IDS, FS, census, dtype_of, forms_of, geom, grain_ok, list_of,
                                make_list, maps_of, operands, reference_bwd, reference_fwd, variant_of)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float('nan')


def _u16():
    from bonai_amd import lib as L
    return (2.0 ** -8, 0.0) if L.act16() == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)


def _round(ref, dt):
    """float64 numpy -> the value rounded ONCE to dt (the reference is representable in fp32 where this is used for equality)."""
    t = torch.from_numpy(np.ascontiguousarray(ref))
    if dt != torch.float32:
        assert torch.equal(t.float().double(), t), 'double rounding'
    return t.float().to(dt).double().numpy()


def _to_dev(a, dt):
    """[N, H, W, C] numpy -> channels_last device tensor [N, C, H, W]."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().permute(0, 3, 1, 2)


def _nan_maps(shapes, dt):
    return [torch.full((b, h, w, c), NAN, dtype=dt, device='cuda').permute(0, 3, 1, 2) for b, c, h, w in shapes]


def _host(t):
    return t.permute(0, 2, 3, 1).double().cpu().numpy()


def _where(a, b):
    return np.argwhere(~(a == b))[:4].tolist()


@functools.lru_cache(maxsize=6)
def _fwd_problem(name, C, kind, n_rot, lattice):
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    feats, _ = operands(name, C, lattice, kind)
    R = reference_fwd(feats, rois, P, hw, strides, n_rot)
    if lattice:
        assert grain_ok(name, R['out'], R['mag'])
    return feats, R


def _run_fwd(name, C, kind, n_rot, variant, ordered, feats):
    from bonai_amd import kernels as K
    rois, P = make_list(name)
    _, strides = maps_of(name)
    dt = dtype_of(kind)
    out = torch.full((n_rot * len(rois), P, P, C), NAN, dtype=dt, device='cuda').permute(0, 3, 1, 2)
    prev = K.ROI_FWD_VARIANT, K.ROI_FWD_SORT_MIN
    K.ROI_FWD_VARIANT, K.ROI_FWD_SORT_MIN = variant, (1 if ordered else None)
    try:
        got = K.roi_align_fwd([_to_dev(f, dt) for f in feats], torch.from_numpy(rois).cuda(), P, strides, FS, n_rot, out=out)
    finally:
        K.ROI_FWD_VARIANT, K.ROI_FWD_SORT_MIN = prev
    assert got is out
    return _host(out)


@pytest.mark.parametrize('row', FORMS, ids=FORM_IDS)
def test_forward_lattice_operands_are_exact(row):
    name = list_of(row)
    feats, R = _fwd_problem(name, row[2], row[3], row[5], True)
    got = _run_fwd(name, row[2], row[3], row[5], variant_of(row), row[7], feats)
    want = _round(R['out'], dtype_of(row[3]))
    assert np.array_equal(got, want), (row[0], _where(got, want))


def test_forward_lattice_one_level_and_crowd():
    """The single-level 16 x 16 map (no level rule; K = 11) and a list of 258 RoIs, through the shipped 16-bit kernel and the fp32 one."""
    for name, C, kind in (('one16', 256, '16'), ('one16', 64, '32'), ('crowd257', 64, '16')):
        feats, R = _fwd_problem(name, C, kind, 1, True)
        got = _run_fwd(name, C, kind, 1, 0, name == 'one16', feats)
        want = _round(R['out'], dtype_of(kind))
        assert np.array_equal(got, want), (name, C, kind, _where(got, want))


@pytest.mark.parametrize('name', ['fine', 'tall', 'wide'])
@pytest.mark.parametrize('kernel', ['sep8_c256', 'sep4_c64', 'sample_f32_c64'])
def test_forward_lattice_fine_and_narrow_maps(name, kernel):
    """'fine': weights of 12 significant bits; 12 RoIs x 2 workgroups = an UNORDERED grid of 24, a multiple of 8: the XCD remap of the
    16-byte kernel without a launch order.  'tall' / 'wide': footprints of 64 rows / columns (the tables' last entry) against 65 (sample loop)."""
    from bonai_amd import kernels as K
    variant, C, kind = {'sep8_c256': (K.ROI_AUTO, 256, '16'), 'sep4_c64': (K.ROI_FWD_SEP4, 64, '16'),
                        'sample_f32_c64': (K.ROI_AUTO, 64, '32')}[kernel]
    n_rot = 4 if name == 'wide' else 1
    feats, R = _fwd_problem(name, C, kind, n_rot, True)
    want = _round(R['out'], dtype_of(kind))
    for ordered in (False, True):
        got = _run_fwd(name, C, kind, n_rot, variant, ordered, feats)
        assert np.array_equal(got, want), (name, kernel, ordered, _where(got, want))


def _fwd_c(row, name):
    """c per RoI row [n_rot K, 1, 1, 1]."""
    from bonai_amd import kernels as K
    rois, P = make_list(name)
    _, strides = maps_of(name)
    forms = forms_of(name, row[2], dtype_of(row[3]), variant_of(row))
    c = []
    for roi, f in zip(rois, forms):
        g = geom(roi, P, strides)
        c.append(max(g['grid_h'], 0) + max(g['grid_w'], 0) + 4 if f[1] == K.ROI_FORM_WALK else 6)
    return np.tile(np.array(c, dtype=np.float64), row[5])[:, None, None, None]


@pytest.mark.parametrize('row', FORMS, ids=FORM_IDS)
def test_forward_random_operands_within_rounding(row):
    name = list_of(row, False)
    feats, R = _fwd_problem(name, row[2], row[3], row[5], False)
    got = _run_fwd(name, row[2], row[3], row[5], variant_of(row), row[7], feats)
    bound = (R['n'] + _fwd_c(row, name)) * U * R['mag']
    if row[3] == '16':
        u16, tiny = _u16()
        bound = bound + u16 * (np.abs(R['out']) + bound) + tiny
    assert np.isfinite(got).all()
    err = np.abs(got - R['out'])
    assert (err[R['mag'] == 0] == 0).all(), 'no term, yet not zero'
    ratio = (err / (bound + 1e-300)).max()
    print(f'ROI_FORM_RATIO fwd {row[0]} {ratio:.4f}')
    assert ratio <= 1.0, (row[0], ratio)


# ---- backward ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=6)
def _bwd_problem(name, C, kind, n_rot, lattice):
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    _, gout = operands(name, C, lattice, kind, n_rot, unit=name.startswith('crowd'))
    G = reference_bwd(gout, rois, P, hw, strides, C, n_rot)
    if lattice:
        for g, m in zip(G['grad'], G['mag']):
            assert grain_ok(name, g, m)
    return gout, G


def _run_bwd(name, C, kind, gkind, n_rot, variant, gout, sort=False, old=None):
    """Write mode into NaN maps, or (old: maps [B, H, W, C] per level) accumulate mode.  sort: the list ordered by image, flagged sorted."""
    from bonai_amd import kernels as K
    rois, P = make_list(name)
    hw, strides = maps_of(name)
    dt, gdt = dtype_of(kind), dtype_of(gkind)
    Kn = len(rois)
    if sort:
        perm = np.argsort(rois[:, 0], kind='stable')
        rois = rois[perm]
        gout = gout.reshape(n_rot, Kn, P, P, C)[:, perm].reshape(n_rot * Kn, P, P, C)
    shapes = [(B, C, h, w) for h, w in hw]
    prev, K.ROI_BWD_VARIANT = K.ROI_BWD_VARIANT, variant
    try:
        kw = dict(grad_feats=[_to_dev(o, gdt) for o in old]) if old is not None else dict(out=_nan_maps(shapes, gdt))
        got = K.roi_align_bwd(_to_dev(gout, dt), torch.from_numpy(rois).cuda(), shapes, P, strides, FS, n_rot, rois_sorted=sort,
                              out_dtype=gdt, **kw)
    finally:
        K.ROI_BWD_VARIANT = prev
    assert all(g.dtype == gdt for g in got)
    return [_host(g) for g in got]


def _old_maps(hw, C, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(-4, 5, (B, h, w, C), generator=gen).double().numpy() for h, w in hw]


@pytest.mark.parametrize('row', BWD_FORMS, ids=BWD_IDS)
def test_backward_lattice_operands_are_exact(row):
    _, variant, C, kind, gkind, P, n_rot, _ = row
    name = 'L' + str(P)
    hw, _ = maps_of(name)
    gout, G = _bwd_problem(name, C, kind, n_rot, True)
    gdt = dtype_of(gkind)
    for sort in (False, True):
        got = _run_bwd(name, C, kind, gkind, n_rot, variant, gout, sort)
        for lv, (g, ref) in enumerate(zip(got, G['grad'])):
            want = _round(ref, gdt)
            assert np.array_equal(g, want), (row[0], 'write', sort, lv, _where(g, want))
        assert not got[3].any() and (not got[0][0].any() if name == 'L7' else True)       # the level / the image without RoIs: zeros
    old = _old_maps(hw, C, 31 + C)
    for sort in (False, True):
        got = _run_bwd(name, C, kind, gkind, n_rot, variant, gout, sort, old)
        for lv, (g, ref, o) in enumerate(zip(got, G['grad'], old)):
            want = _round(o + ref, gdt)
            assert np.array_equal(g, want), (row[0], 'accumulate', sort, lv, _where(g, want))


@pytest.mark.parametrize('n_rot', [1, 4])
@pytest.mark.parametrize('form', ['valu_16', 'mfma', 'pipe'])
def test_backward_fine_lattice_needs_both_weight_pieces(form, n_rot):
    """List 'fine': weights on the 1 / 64 lattice need up to 12 significant bits (test_census_fine), more than one 16-bit piece of
    the MFMA kernels' two-piece weight holds, while every sum stays exact in fp32: a kernel that drops or mis-rounds the low piece
    cannot return the reference."""
    from bonai_amd import kernels as K
    variant = {'valu_16': K.ROI_BWD_VALU, 'mfma': K.ROI_AUTO, 'pipe': K.ROI_BWD_PIPE}[form]
    hw, _ = maps_of('fine')
    gout, G = _bwd_problem('fine', 256, '16', n_rot, True)
    gdt = dtype_of('16')
    old = _old_maps(hw, 256, 5)
    for sort in (False, True):
        got = _run_bwd('fine', 256, '16', '16', n_rot, variant, gout, sort)
        acc = _run_bwd('fine', 256, '16', '16', n_rot, variant, gout, sort, old)
        for lv, (g, a, ref, o) in enumerate(zip(got, acc, G['grad'], old)):
            assert np.array_equal(g, _round(ref, gdt)), (form, 'write', sort, lv, _where(g, _round(ref, gdt)))
            assert np.array_equal(a, _round(o + ref, gdt)), (form, 'accumulate', sort, lv)


@pytest.mark.parametrize('name', ['crowd257', 'crowd513', 'one16'])
@pytest.mark.parametrize('form', ['valu_f32', 'valu_16', 'mfma', 'pipe'])
def test_backward_lattice_crowds_and_one_level(name, form):
    """> 256 RoIs of one image on one tile (two and three batches of the tile owner's list; gradients in {0, +-1}), and the one-level
    16 x 16 map whose 8 tiles switch the MFMA kernel's XCD remap on."""
    from bonai_amd import kernels as K
    variant, C, kind, gkind = {'valu_f32': (K.ROI_AUTO, 64, '32', '32'), 'valu_16': (K.ROI_BWD_VALU, 256, '16', '16'),
                               'mfma': (K.ROI_AUTO, 256, '16', '16'), 'pipe': (K.ROI_BWD_PIPE, 256, '16', '16')}[form]
    gout, G = _bwd_problem(name, C, kind, 1, True)
    for sort in (False, True):
        got = _run_bwd(name, C, kind, gkind, 1, variant, gout, sort)
        for lv, (g, ref) in enumerate(zip(got, G['grad'])):
            want = _round(ref, dtype_of(gkind))
            assert np.array_equal(g, want), (name, form, sort, lv, _where(g, want))


@pytest.mark.parametrize('row', BWD_FORMS, ids=BWD_IDS)
def test_backward_random_operands_within_rounding(row):
    _, variant, C, kind, gkind, P, n_rot, kern = row
    name = 'R' + str(P)
    rois, _ = make_list(name)
    _, strides = maps_of(name)
    gout, G = _bwd_problem(name, C, kind, n_rot, False)
    got = _run_bwd(name, C, kind, gkind, n_rot, variant, gout)
    gsum = max(max(geom(r, P, strides)['grid_h'], 0) + max(geom(r, P, strides)['grid_w'], 0) for r in rois)
    u16, tiny = _u16()
    worst = 0.0
    for lv, (g, ref, mag, n) in enumerate(zip(got, G['grad'], G['mag'], G['n'])):
        if kern in ('mfma', 'pipe'):
            bound = (2 * n + gsum + 3) * U * mag + 2.0 ** -16 * mag + (u16 * mag if n_rot == 4 else 0)
        else:
            bound = (n + gsum + 4 + (n_rot - 1)) * U * mag
        if gkind == '16':
            bound = bound + u16 * (np.abs(ref) + bound) + tiny
        assert np.isfinite(g).all(), (row[0], lv)
        err = np.abs(g - ref)
        assert (err[mag == 0] == 0).all(), 'no term, yet not zero'
        worst = max(worst, (err / (bound + 1e-300)).max())
    print(f'ROI_FORM_RATIO bwd {row[0]} {worst:.4f}')
    assert worst <= 1.0, (row[0], worst)


def _multi_sets(specs, C, lattice=True):
    """specs: [(list name | None for an empty list, n_rot)] -> (sets for K.roi_align_bwd_multi, [reference maps per list])."""
    from bonai_amd import lib as L
    sets, refs = [], []
    for name, n_rot in specs:
        if name is None:
            sets.append((torch.zeros(0, 14, 14, C, dtype=L.act16(), device='cuda').permute(0, 3, 1, 2), torch.zeros(0, 5, device='cuda'),
                         14, 1, True))
            continue
        rois, P = make_list(name)
        gout, G = _bwd_problem(name, C, '16', n_rot, lattice)
        perm = np.argsort(rois[:, 0], kind='stable')
        g = gout.reshape(n_rot, len(rois), P, P, C)[:, perm].reshape(-1, P, P, C)
        sets.append((_to_dev(g, L.act16()), torch.from_numpy(rois[perm]).cuda(), P, n_rot, True))
        refs.append(G['grad'])
    return sets, refs


@pytest.mark.parametrize('specs', [(('L7', 1),), (('L7', 1), ('L14', 1)), (('L7', 1), (None, 1), ('L14', 4)), (('L14', 1), ('L7', 4), ('L7', 1)),
                                   (('fine', 1),), (('fine', 4), ('L14', 1), ('fine', 1))],
                         ids=['one', 'two', 'three_with_an_empty_one', 'three', 'fine', 'fine_in_three'])
def test_multi_list_lattice_operands_are_exact(specs):
    """loft_roi_align_bwd_multi, fused (C = 256, 16-bit maps, <= 3 lists): the exact sum of the lists' maps, rounded once; one list is
    bit for bit roi_align_bwd; accumulate mode adds the old 16-bit value before the one rounding."""
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    C = 256
    hw, strides = maps_of('L7')
    shapes = [(B, C, h, w) for h, w in hw]
    sets, refs = _multi_sets(specs, C)
    total = [sum(r[lv] for r in refs) for lv in range(4)]
    got = K.roi_align_bwd_multi(sets, shapes, strides, FS, out=_nan_maps(shapes, L.act16()))
    for lv in range(4):
        want = _round(total[lv], L.act16())
        assert np.array_equal(_host(got[lv]), want), ('write', lv, _where(_host(got[lv]), want))
    old = _old_maps(hw, C, 77)
    acc = K.roi_align_bwd_multi(sets, shapes, strides, FS, grad_feats=[_to_dev(o, L.act16()) for o in old])
    for lv in range(4):
        want = _round(old[lv] + total[lv], L.act16())
        assert np.array_equal(_host(acc[lv]), want), ('accumulate', lv)
    if len(specs) == 1:
        g, rois, P, n_rot, _ = sets[0]
        one = K.roi_align_bwd(g, rois, shapes, P, strides, FS, n_rot, rois_sorted=True, out_dtype=L.act16(), out=_nan_maps(shapes, L.act16()))
        assert all(torch.equal(a, b) for a, b in zip(one, got))


def test_a_fourth_list_goes_list_after_list():
    """Four lists: the library runs them one after another, the later ones accumulating -- each pass rounds the 16-bit map once."""
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    C = 256
    hw, strides = maps_of('L7')
    shapes = [(B, C, h, w) for h, w in hw]
    sets, refs = _multi_sets((('L7', 1), ('L14', 1), ('L7', 4), ('L14', 4)), C)
    got = K.roi_align_bwd_multi(sets, shapes, strides, FS, out=_nan_maps(shapes, L.act16()))
    for lv in range(4):
        cur = np.zeros_like(refs[0][lv])
        for r in refs:
            cur = _round(cur + r[lv], L.act16())
        assert np.array_equal(_host(got[lv]), cur), (lv, _where(_host(got[lv]), cur))


def test_multi_list_random_operands_within_rounding():
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    C = 256
    hw, strides = maps_of('R7')
    shapes = [(B, C, h, w) for h, w in hw]
    specs = (('R7', 1), ('R14', 1), ('R7', 4))
    sets, refs = _multi_sets(specs, C, False)
    got = K.roi_align_bwd_multi(sets, shapes, strides, FS, out=_nan_maps(shapes, L.act16()))
    u16, tiny = _u16()
    gsum = 0
    for name, _ in specs:
        rois, P = make_list(name)
        gsum = max(gsum, max(max(geom(r, P, strides)['grid_h'], 0) + max(geom(r, P, strides)['grid_w'], 0) for r in rois))
    worst = 0.0
    for lv in range(4):
        ref = sum(r[lv] for r in refs)
        mag = sum(_bwd_problem(n, C, '16', rot, False)[1]['mag'][lv] for n, rot in specs)
        mag4 = _bwd_problem('R7', C, '16', 4, False)[1]['mag'][lv]
        n = sum(_bwd_problem(nm, C, '16', rot, False)[1]['n'][lv] for nm, rot in specs)
        bound = (2 * n + gsum + 3) * U * mag + 2.0 ** -16 * mag + u16 * mag4
        bound = bound + u16 * (np.abs(ref) + bound) + tiny
        g = _host(got[lv])
        assert np.isfinite(g).all()
        worst = max(worst, (np.abs(g - ref) / (bound + 1e-300)).max())
    print(f'ROI_FORM_RATIO bwd multi_three_lists {worst:.4f}')
    assert worst <= 1.0, worst


# ---- (C) dispatch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,n_rot', [('R7', 1), ('R14', 4), ('L7', 1), ('fine', 1)])
def test_auto_is_the_form_each_roi_resolves_to(name, n_rot):
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    C = 256
    rois, P = make_list(name)
    feats, _ = _fwd_problem(name, C, '16', n_rot, False)
    auto = _run_fwd(name, C, '16', n_rot, K.ROI_AUTO, False, feats)
    staged = _run_fwd(name, C, '16', n_rot, K.roi_fwd_variant(stage_kib=64, gmax=15), False, feats)
    streamed = _run_fwd(name, C, '16', n_rot, K.roi_fwd_variant(stage_kib=255), False, feats)
    forms = forms_of(name, C, L.act16())
    differ = 0
    for k, f in enumerate(forms):
        rows = [r * len(rois) + k for r in range(n_rot)]
        want, other = (staged, streamed) if f[1] == K.ROI_FORM_LDS else (streamed, staged)
        assert np.array_equal(auto[rows], want[rows]), (name, k, f)
        differ += int(not np.array_equal(auto[rows], other[rows]))
    if name.startswith('R'):    # off the lattice the two forced launches do differ where the forms' sum orders differ (on it both are exact)
        assert differ >= 3
    for ns in (1, 2, 3):
        assert np.array_equal(auto, _run_fwd(name, C, '16', n_rot, K.roi_fwd_variant(nsplit=ns), False, feats)), ns
        assert np.array_equal(auto, _run_fwd(name, C, '16', n_rot, K.roi_fwd_variant(nsplit=ns), True, feats)), (ns, 'ordered')
    assert name == 'fine' or (census(name)['walk'] >= 1 and census(name)['lds'])      # ('fine': 12 x nsplit 2 = an unordered grid of 24)
