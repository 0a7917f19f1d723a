"""CPU: which kernel the DCNv2 sampling backward takes for a shape (loft_mdcn_bwd_form, a host-only query of the launch path
itself), and what loft_mdcn_sample_bwd_v refuses.  FORMS holds one row per kernel form (family x channels per lane / split count
x reduction shape) -- the table tests/test_deform_forms_gpu.py runs at the GEOS geometries; PRODUCTION pins what LOFT_MDCN_AUTO
gives the maps of the config-4 model at batch 8 x 1024^2, with the workspace bytes of the dispatch rule written out: moving a
threshold of the rule fails here, without a GPU."""
import os

import pytest
import torch

from bonai_amd import kernels as K
from bonai_amd import lib as L

# name -> (IH, IW, k, stride, pad, dil).  19 x 17: rectangular, neither a multiple of the 8- or 4-pixel tile edge
GEOS = {
    's1': (19, 17, 3, 1, 1, 1),        # 19 x 17 outputs: 3 x 3 tiles of 8 x 8, the last row / column of tiles 3 / 1 pixels wide
    's2': (19, 17, 3, 2, 1, 1),        # 10 x 9 outputs: 3 x 3 tiles of 4 x 4
    'k1': (19, 17, 1, 1, 0, 1),        # one tap
    'part': (5, 3, 3, 1, 1, 1),        # one partial tile
    'tiny': (6, 6, 3, 1, 1, 1),        # the 1024-channel row's map
    'dil2': (19, 17, 3, 1, 2, 2),      # dilation: generic kernel only
}
BASE = ('s1', 's2', 'k1', 'part')
B = 2

# (id, operand type '16' | '32', C, deform groups, family, count (CPL of the binned / splits of the window kernel), offmask channels
#  padded to a multiple of 4, geometries)
FORMS = [
    ('bin_c64_cpl1', '16', 64, 1, 'BIN', 1, True, BASE),
    ('bin_c128_cpl1_2slabs', '16', 128, 1, 'BIN', 1, False, BASE),
    ('bin_c128_cpl2', '16', 128, 1, 'BIN', 2, False, BASE),
    ('bin_c256_cpl4', '16', 256, 1, 'BIN', 4, False, BASE),
    ('bin_c256_cpl2_2slabs', '16', 256, 1, 'BIN', 2, True, BASE),
    ('bin_c512_cpl8', '16', 512, 1, 'BIN', 8, False, BASE),
    ('bin_c512_cpl4_2slabs', '16', 512, 1, 'BIN', 4, False, BASE),
    ('bin_c192_cpl1_3slabs', '16', 192, 1, 'BIN', 1, False, BASE),
    ('tile_c64_splits1', '32', 64, 1, 'TILE', 1, True, BASE),
    ('tile_c256_splits1', '32', 256, 1, 'TILE', 1, False, BASE),       # one workgroup walks four chunks
    ('tile_c256_splits2', '32', 256, 1, 'TILE', 2, True, BASE),
    ('tile_c256_splits4', '32', 256, 1, 'TILE', 4, False, BASE),
    ('tile_c192_splits2', '32', 192, 1, 'TILE', 2, False, BASE),       # chunks 0, 2 | 1
]
for _t in ('32', '16'):
    FORMS += [
        (f'generic{_t}_c64_dg1_seg8', _t, 64, 1, 'GENERIC', 0, False, BASE),
        (f'generic{_t}_c64_dg2_seg4', _t, 64, 2, 'GENERIC', 0, True, BASE),
        (f'generic{_t}_c512_dg1_wave', _t, 512, 1, 'GENERIC', 0, False, BASE),
        (f'generic{_t}_c1024_dg1_lds', _t, 1024, 1, 'GENERIC', 0, False, ('tiny',)),
        (f'generic{_t}_c128_dg4', _t, 128, 4, 'GENERIC', 0, False, BASE),
        (f'generic{_t}_c72_lanewise', _t, 72, 1, 'GENERIC', 0, False, ('s1', 'part')),     # 9 lanes per item: no power of two
        (f'generic{_t}_c64_dil2', _t, 64, 1, 'GENERIC', 0, False, ('dil2',)),
    ]
CASES = [(row, geo) for row in FORMS for geo in row[7]]
CASE_IDS = [f'{row[0]}-{geo}' for row, geo in CASES]

FAMILY = {'GENERIC': K.MDCN_BWD_GENERIC, 'TILE': K.MDCN_BWD_TILE, 'BIN': K.MDCN_BWD_BIN}


def dtype_of(kind):
    return torch.float32 if kind == '32' else L.act16()


def geometry(geo, C, DG=1, padded=False):
    """-> the shape arguments of K.mdcn_bwd_form for FORMS geometry `geo`."""
    IH, IW, k, stride, pad, dil = GEOS[geo]
    OH, OW = (IH + 2 * pad - dil * (k - 1) - 1) // stride + 1, (IW + 2 * pad - dil * (k - 1) - 1) // stride + 1
    nch = 3 * DG * k * k
    return dict(B=B, IH=IH, IW=IW, C=C, OH=OH, OW=OW, kh=k, kw=k, stride=stride, pad=pad, dil=dil, deform_groups=DG,
                omc=(nch + 3) // 4 * 4 if padded else nch)


def variant_of(row):
    return K.mdcn_variant(FAMILY[row[4]], row[5])


def expected_form(row, geo):
    """(family, count, tile edge) the row names."""
    if row[4] == 'GENERIC':
        return (K.MDCN_BWD_GENERIC, 0, 0)
    return (FAMILY[row[4]], row[5], 8 if GEOS[geo][3] == 1 else 4)


@pytest.fixture(scope='module', autouse=True)
def _library():
    if not (os.path.exists(L._LIB_PATH) and os.path.exists(L._LIB_PATH_F16)):
        from bonai_amd import build
        build.build()


def test_codes():
    assert (K.MDCN_AUTO, K.MDCN_BWD_GENERIC, K.MDCN_BWD_TILE, K.MDCN_BWD_BIN) == (0, 1, 2, 3)
    assert K.mdcn_variant(K.MDCN_BWD_BIN, 4) == 3 | 4 << 8


# ---- (a) the production shapes under AUTO: config 4 (DCNv2 in ResNet c3-c5 and the FPN) at batch 8 x 1024^2, 3 x 3 kernels.
# Read off mdcn_tiling: tiles = B * ceil(OH / T) * ceil(OW / T), T = 8 at stride 1 and 4 at stride 2; splits =
# clamp(ceil(1024 / tiles), 1, C / 64); CPL = the largest of 8, 4, 2, 1 that is <= C / 64 and divides it, halved while
# tiles * (C / 64 / CPL) < 1024.
# (B, C, IH, OH, stride, tile edge, tiles, CPL, slabs, splits, window edge)
PRODUCTION = [
    (8, 256, 256, 256, 1, 8, 8192, 4, 1, 1, 15),       # FPN P2
    (8, 256, 64, 64, 1, 8, 512, 2, 2, 2, 15),          # FPN P4
    (8, 512, 32, 32, 1, 8, 128, 1, 8, 8, 15),          # layer4
    (8, 128, 256, 128, 2, 4, 8192, 2, 1, 1, 14),       # layer2, first block: stride 2
    (2, 128, 14, 14, 1, 8, 8, 1, 2, 2, 15),            # the composed-op test's shape
]


@pytest.mark.parametrize('row', PRODUCTION, ids=[f'b{r[0]}_c{r[1]}_o{r[3]}_s{r[4]}' for r in PRODUCTION])
@pytest.mark.parametrize('omc', [27, 28])
def test_auto_on_the_production_shapes(row, omc):
    Bn, C, IH, OH, stride, edge, tiles, cpl, nslab, splits, win = row
    assert tiles == Bn * (-(-OH // edge)) ** 2 and nslab == C // 64 // cpl
    shape = dict(B=Bn, IH=IH, IW=IH, C=C, OH=OH, OW=OH, kh=3, kw=3, stride=stride, pad=1, dil=1, deform_groups=1, omc=omc)
    assert K.mdcn_bwd_form(dtype=L.act16(), **shape) == (K.MDCN_BWD_BIN, cpl, edge)
    assert K.mdcn_bwd_form(dtype=torch.float32, **shape) == (K.MDCN_BWD_TILE, splits, edge)
    # the forced form with AUTO's own count (0) resolves to the same kernel
    assert K.mdcn_bwd_form(dtype=L.act16(), variant=K.mdcn_variant(K.MDCN_BWD_BIN), **shape) == (K.MDCN_BWD_BIN, cpl, edge)
    assert K.mdcn_bwd_form(dtype=torch.float32, variant=K.mdcn_variant(K.MDCN_BWD_TILE), **shape) == (K.MDCN_BWD_TILE, splits, edge)
    # workspace: one fp32 window of win x win pixels per (tile, 64-channel chunk) + a doffmask copy per split / slab when > 1
    lib = L.load()
    windows = tiles * (C // 64) * win * win * 64
    M = Bn * OH * OH
    parts = max(splits, nslab)
    want = 4 * (windows + (parts * M * omc if parts > 1 else 0))
    args = (Bn, C, OH, OH, 3, 3, stride, 1, 1, omc)
    assert lib.loft_mdcn_bwd_workspace_bytes(*args) == want
    assert lib.loft_mdcn_bwd_workspace_bytes_v(*args, K.MDCN_AUTO) == want
    assert lib.loft_mdcn_bwd_workspace_bytes_v(*args, K.mdcn_variant(K.MDCN_BWD_BIN)) == \
        4 * (windows + (nslab * M * omc if nslab > 1 else 0))
    assert lib.loft_mdcn_bwd_workspace_bytes_v(*args, K.mdcn_variant(K.MDCN_BWD_TILE, C // 64)) == \
        4 * (windows + (C // 64 * M * omc if C > 64 else 0))
    assert lib.loft_mdcn_bwd_workspace_bytes_v(*args, K.MDCN_BWD_GENERIC) == 0


@pytest.mark.parametrize('change', [dict(deform_groups=2, omc=54), dict(C=72), dict(C=32), dict(C=96, deform_groups=3, omc=81), dict(dil=2, pad=2),
                                    dict(stride=3, OH=86, OW=86)], ids=['dg2', 'c72', 'c32', 'c96_dg3', 'dil2', 'window_17'])
def test_auto_takes_the_generic_kernel(change):
    shape = dict(B=8, IH=256, IW=256, C=256, OH=256, OW=256, kh=3, kw=3, stride=1, pad=1, dil=1, deform_groups=1, omc=27)
    shape.update(change)
    for dt in (torch.float32, L.act16()):
        assert K.mdcn_bwd_form(dtype=dt, **shape) == (K.MDCN_BWD_GENERIC, 0, 0)
    s = shape
    assert L.load().loft_mdcn_bwd_workspace_bytes(s['B'], s['C'], s['OH'], s['OW'], 3, 3, s['stride'], s['dil'], s['deform_groups'],
                                                  s['omc']) == 0


# ---- (b) every row of the GPU table reports the form it forces
@pytest.mark.parametrize('row,geo', CASES, ids=CASE_IDS)
def test_forced_row_reports_its_form(row, geo):
    shape = geometry(geo, row[2], row[3], row[6])
    assert K.mdcn_bwd_form(dtype=dtype_of(row[1]), variant=variant_of(row), **shape) == expected_form(row, geo)
    nws = L.load().loft_mdcn_bwd_workspace_bytes_v(B, row[2], shape['OH'], shape['OW'], shape['kh'], shape['kw'], shape['stride'],
                                                   shape['dil'], row[3], shape['omc'], variant_of(row))
    assert (nws == 0) if row[4] == 'GENERIC' else (nws > 0)


def test_table_reaches_every_kernel_form():
    got = {(r[4], r[5]) for r in FORMS}
    assert {('BIN', c) for c in (1, 2, 4, 8)} <= got and {('TILE', s) for s in (1, 2, 4)} <= got
    # the generic kernel's three reductions: segments shorter than a wave, one wave, several waves (C / 8 / DG vs 64)
    cpg = {r[2] // 8 // r[3] for r in FORMS if r[4] == 'GENERIC'}
    assert min(cpg) < 64 and 64 in cpg and max(cpg) > 64


def test_both_builds_choose_the_same_form():
    prev = L.set_act16(torch.float16)
    try:
        f16 = [K.mdcn_bwd_form(dtype=dtype_of(r[1]), variant=variant_of(r), **geometry(g, r[2], r[3], r[6])) for r, g in CASES]
    finally:
        L.set_act16(prev)
    assert f16 == [expected_form(r, g) for r, g in CASES]


# ---- (c) refusals: hipErrorInvalidValue (1), from the form query, the workspace query and the launch alike
def _launch_code(shape, dtype_code, variant, workspace=True):
    """The return code of loft_mdcn_sample_bwd_v.  A refusal returns before anything is launched or dereferenced, so without a
    device the buffers are made-up host addresses; where a device is present they are real and large enough for any form of the
    shape, so that a refusal that regressed shows as a failed assert and not as a kernel on wild pointers."""
    s = shape
    M, KK = s['B'] * s['OH'] * s['OW'], s['kh'] * s['kw']
    if torch.cuda.is_available():
        f = lambda n: torch.zeros(n, dtype=torch.float32, device='cuda')      # noqa: E731  (fp32 sizes cover the 16-bit operands)
        bufs = [f(s['B'] * s['IH'] * s['IW'] * s['C']), f(M * s['omc']), f(M * KK * s['C']), f(s['B'] * s['IH'] * s['IW'] * s['C']),
                f(M * s['omc'])]
        tiles = s['B'] * -(-s['OH'] // 4) * -(-s['OW'] // 4)
        ws = f(tiles * -(-s['C'] // 64) * 225 * 64 + 32 * M * s['omc'])
        ptrs = [b.data_ptr() for b in bufs] + [ws.data_ptr() if workspace else None]
    else:
        ptrs = [1 << 20] * 5 + [1 << 20 if workspace else None]
    code = L.load().loft_mdcn_sample_bwd_v(*ptrs[:5], dtype_code, s['B'], s['IH'], s['IW'], s['C'], s['OH'], s['OW'], s['kh'], s['kw'],
                                           s['stride'], s['pad'], s['dil'], s['deform_groups'], s['omc'], ptrs[5], variant, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return code


REFUSALS = [
    ('bin_on_fp32', 's1', 128, 1, '32', ('BIN', 1)),
    ('tile_on_16bit', 's1', 128, 1, '16', ('TILE', 1)),
    ('cpl2_on_three_chunks', 's1', 192, 1, '16', ('BIN', 2)),
    ('cpl4_on_two_chunks', 's1', 128, 1, '16', ('BIN', 4)),
    ('cpl3', 's1', 192, 1, '16', ('BIN', 3)),
    ('cpl16', 's1', 1024, 1, '16', ('BIN', 16)),
    ('bin_dg2', 's1', 128, 2, '16', ('BIN', 1)),
    ('tile_dg2', 's1', 128, 2, '32', ('TILE', 1)),
    ('bin_dil2', 'dil2', 128, 1, '16', ('BIN', 1)),
    ('tile_dil2', 'dil2', 128, 1, '32', ('TILE', 1)),
    ('bin_c32', 's1', 32, 1, '16', ('BIN', 1)),
    ('tile_c32', 's1', 32, 1, '32', ('TILE', 1)),
    ('tile_splits_over_chunks', 's1', 256, 1, '32', ('TILE', 5)),
    ('generic_with_count', 's1', 128, 1, '32', ('GENERIC', 2)),
]


@pytest.mark.parametrize('case', REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case):
    _, geo, C, DG, kind, (fam, count) = case
    shape = geometry(geo, C, DG)
    v = K.mdcn_variant(FAMILY[fam], count)
    with pytest.raises(L.LoftHipError):
        K.mdcn_bwd_form(dtype=dtype_of(kind), variant=v, **shape)
    assert _launch_code(shape, L._DT[dtype_of(kind)], v) == 1
    # the shape is fine under AUTO and as the generic kernel
    assert K.mdcn_bwd_form(dtype=dtype_of(kind), **shape)[0] in FAMILY.values()
    assert K.mdcn_bwd_form(dtype=dtype_of(kind), variant=K.MDCN_BWD_GENERIC, **shape) == (K.MDCN_BWD_GENERIC, 0, 0)


def test_refusals_of_codes_and_windows():
    shape = geometry('s1', 128)
    for v in (4, 255, K.mdcn_variant(K.MDCN_AUTO, 2), 1 << 16 | K.MDCN_BWD_TILE, -1):      # unknown family / stray bits
        with pytest.raises(L.LoftHipError):
            K.mdcn_bwd_form(dtype=torch.float32, variant=v, **shape)
        assert _launch_code(shape, L.F32, v) == 1
        assert L.load().loft_mdcn_bwd_workspace_bytes_v(B, 128, 19, 17, 3, 3, 1, 1, 1, 27, v) == -1
    # stride 3: the 8 x 8 tile's window would be 17 x 17 > 15 x 15
    wide = dict(B=2, IH=19, IW=17, C=128, OH=7, OW=6, kh=3, kw=3, stride=3, pad=1, dil=1, deform_groups=1, omc=27)
    for kind, fam in (('32', K.MDCN_BWD_TILE), ('16', K.MDCN_BWD_BIN)):
        with pytest.raises(L.LoftHipError):
            K.mdcn_bwd_form(dtype=dtype_of(kind), variant=fam, **wide)
        assert _launch_code(wide, L._DT[dtype_of(kind)], fam) == 1
        assert L.load().loft_mdcn_bwd_workspace_bytes_v(2, 128, 7, 6, 3, 3, 3, 1, 1, 27, fam) == -1
    # a tiled family without a workspace, the other build's 16-bit type
    assert _launch_code(shape, L.F32, K.MDCN_BWD_TILE, workspace=False) == 1
    other = L.F16 if L.act16() == torch.bfloat16 else L.BF16
    assert _launch_code(shape, other, K.MDCN_AUTO) == 1
    assert L.load().loft_mdcn_bwd_form(2, 19, 17, 128, 19, 17, 3, 3, 1, 1, 1, 1, 27, other, 0) == -1
