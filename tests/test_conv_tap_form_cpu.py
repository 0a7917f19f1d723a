"""CPU: which kernel the forward / data-gradient tap convolution takes for a launch (K.conv_tap_form -> loft_conv_tap_form, a
host-only query of conv_tap_plan, the function the launches themselves call).  Four things are pinned without a GPU:
  - the launch refuses exactly what serves() of tests/test_conv_forms_cpu.py says it refuses, for every case of that file's
    tables, and the head / operand-plane launches refuse what include/loft_hip.h says;
  - LOFT_CONV_AUTO: one shape on either side of every threshold of the dispatcher, each with the kernel and tile it was written
    for (the expected values are the rule of include/loft_hip.h and DESIGN.md worked out by hand -- see AUTO_ROWS) -- a moved
    threshold fails here instead of silently leaving the GPU file's cases, and the model, on another kernel;
  - the pixel-major flag and the padded row count of the RoI geometries;
  - the instance a STREAM256 launch takes under every process-wide stream form."""
import contextlib
import os

import pytest
import torch  # noqa: F401  (load torch's HIP runtime before libloft_hip.so)

from bonai_amd import kernels as K
from bonai_amd import lib as L
from test_conv_forms_cpu import (EPI, GEO, GEOMETRIES, KERNELS, LOCKSTEP, PIPELINED, ROI_GEOS, _serves_launch, cases_of, epilogues_of,
                                 variant_code)


@pytest.fixture(scope='module', autouse=True)
def _library():
    if not (os.path.exists(L._LIB_PATH) and os.path.exists(L._LIB_PATH_F16)):
        from bonai_amd import build
        build.build()


@contextlib.contextmanager
def stream_form(form):
    lib = L.load()
    prev = lib.loft_conv_stream_form(form)
    try:
        yield
    finally:
        lib.loft_conv_stream_form(prev)


def code(name):
    return getattr(K, 'CONV_' + name)


def name_of(c):
    return KERNELS[c] if 0 <= c < len(KERNELS) else c


def query(geo, la, epi=EPI['plain'], variant=K.CONV_AUTO, **kw):
    """The query for launch `la` of a tests/test_conv_forms_cpu.py geometry with epilogue `epi`."""
    return K.conv_tap_form(geo.B, geo.IH, geo.IW, geo.Cin, geo.Cout, la.OH, la.OW, geo.OHf, geo.OWf, list(la.taps), ss=la.ss, os=la.os,
                           oo=(la.oo_y, la.oo_x), out_f32=epi.f32, accumulate=epi.accumulate, groups=geo.G, variant=variant,
                           residual=epi.residual, mask=epi.mask, **kw)


def refused(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except L.LoftHipError as e:
        assert 'hipError_t 1' in str(e), e              # hipErrorInvalidValue, nothing else
        return True
    return False


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize('geo', GEOMETRIES, ids=lambda g: g.id)
def test_launch_refuses_exactly_what_serves_says(geo):
    """Every (epilogue, kernel / flag / stream-form case) the GPU file runs on this geometry, every launch of it."""
    checked = 0
    for epi in epilogues_of(geo):
        for c in cases_of(geo, epi):
            with stream_form(c.form if c.form is not None else -1):
                for la in geo.launches:
                    want = _serves_launch(c.kernel, c.flags, geo, la, epi)
                    assert refused(query, geo, la, epi, variant_code(c)) == (not want), (geo.id, epi.id, c.id, la)
                    checked += 1
    assert checked >= 20 * len(geo.launches)


def test_a_served_launch_reports_the_pinned_kernel_and_its_tile():
    """A pinned code comes back as itself (form 0: no stream form to resolve) with the tile include/loft_hip.h gives it."""
    tiles = {'PIPE256': (256, 256), 'T256_FAST': (256, 256), 'T256': (256, 256), 'T128_SINGLE': (128, 128), 'T128_FAST': (128, 128),
             'T128': (128, 128), 'T128x64': (128, 64), 'PATCH64': (256, 64), 'STREAM256': (256, 256), 'STREAM128': (128, 256),
             'STREAM64': (64, 256), 'STREAM64N': (64, 128), 'ROLES256': (256, 256), 'STREAM256N': (256, 128), 'RING32': (256, 256),
             'W4': (256, 256), 'XFIRST': (256, 256), 'LEAN': (256, 256), 'LEANX': (256, 256)}
    assert set(tiles) == set(KERNELS) - {'AUTO'}
    with stream_form(0):
        for k, tile in tiles.items():
            geo = GEO['p64_3x3_ragged'] if k == 'PATCH64' else GEO['fwd3x3_ragged']
            f = query(geo, geo.launches[0], EPI['bias_relu'], code(k))
            assert (name_of(f.kernel), f.tile_pixels, f.tile_couts) == (k, *tile), (k, f)
        geo = GEO['fwd3x3_s2_n128']                      # Cout = 128: STREAM256's 128-cout tiles
        f = query(geo, geo.launches[0], EPI['bias_relu'], K.CONV_STREAM256)
        assert (name_of(f.kernel), f.tile_pixels, f.tile_couts) == ('STREAM256', 256, 128)


def test_no_output_pixel_is_no_launch_and_bad_arguments_are_refused():
    geo = GEO['fwd3x3_ragged']
    la = geo.launches[0]
    assert query(geo._replace(B=0), la).kernel == 0
    assert refused(query, geo._replace(Cin=96), la) and refused(query, geo._replace(Cout=254), la) and refused(query, geo._replace(G=0), la)
    assert refused(query, geo, la._replace(taps=la.taps * 2))                        # 18 taps > CONV_MAX_TAPS
    assert refused(query, geo, la, variant=20) and refused(query, geo, la, variant=K.CONV_STREAM256 | 0x40000)
    # experiment bits 12-15: instances of PIPE256 and of STREAM256's 256 x 256 tile only, and only the compiled ones
    assert not refused(query, geo, la, variant=K.CONV_STREAM256 | (2 << 12)) and refused(query, geo, la, variant=K.CONV_STREAM256 | (5 << 12))
    assert not refused(query, geo, la, variant=K.CONV_PIPE256 | (5 << 12)) and refused(query, geo, la, variant=K.CONV_PIPE256 | (2 << 12))
    assert refused(query, geo, la, variant=K.CONV_STREAM128 | (1 << 12)) and refused(query, geo, la, variant=K.CONV_LEAN | (1 << 12))
    n128 = GEO['fwd3x3_s2_n128']
    assert refused(query, n128, n128.launches[0], variant=K.CONV_STREAM256 | (1 << 12))
    assert not refused(query, geo, la, variant=K.CONV_T128 | (1 << 12))              # (the lockstep kernels ignore them)


# the bench's 3x3 conv of the RPN on P2 -- 2048 pixel tiles: what a head launch is served on
BIG = dict(B=8, IH=256, IW=256, Cin=256, Cout=256, OH=256, OW=256, OHf=256, OWf=256,
           taps=[(r - 1, s - 1, r * 3 + s) for r in range(3) for s in range(3)])


def test_head_launches_are_refused_as_the_header_says():
    """loft_conv_tap_bf16_head: Cout == 256, one group, 16-bit output, no mask, the library's own choice, and only where that
    choice is a 256-cout stream tile; 4 <= head_c4 <= 32, a multiple of 4."""
    with stream_form(2):
        f = K.conv_tap_form(**BIG, head_c4=16)
        assert (name_of(f.kernel), f.tile_pixels, f.tile_couts) == ('LEAN', 256, 256)
    assert not refused(K.conv_tap_form, **BIG, head_c4=4) and not refused(K.conv_tap_form, **BIG, head_c4=32, residual=True)
    for c4 in (2, 6, 36):
        assert refused(K.conv_tap_form, **BIG, head_c4=c4), c4
    assert refused(K.conv_tap_form, **BIG, head_c4=16, mask=True)
    assert refused(K.conv_tap_form, **BIG, head_c4=16, out_f32=True) and refused(K.conv_tap_form, **BIG, head_c4=16, groups=2)
    assert refused(K.conv_tap_form, **dict(BIG, Cout=512), head_c4=16)
    assert refused(K.conv_tap_form, **BIG, head_c4=16, variant=K.CONV_AUTO | K.CONV_FLAG_KROT)
    for k in KERNELS[1:]:                                # a pinned code: the three stream tiles of 256 couts only
        assert refused(K.conv_tap_form, **BIG, head_c4=16, variant=code(k)) == (k not in ('STREAM256', 'STREAM128', 'STREAM64')), k
    # the dispatcher leaves a small launch on a lockstep kernel (646 rows: T128), which has no head epilogue
    geo = GEO['fwd3x3_ragged']
    assert name_of(query(geo, geo.launches[0]).kernel) == 'T128' and refused(query, geo, geo.launches[0], head_c4=16)
    assert not refused(query, geo, geo.launches[0], variant=K.CONV_STREAM64, head_c4=16)


def test_plane_launches_are_refused_as_the_header_says():
    """loft_conv_tap_planes: Cout % 128 == 0, Cin % 64 == 0, nterms <= 8, nterms * T <= 64."""
    assert not refused(K.conv_tap_form, **BIG, nterms=6) and not refused(K.conv_tap_form, **BIG, nterms=7)      # 63 (term, tap) pairs
    assert refused(K.conv_tap_form, **BIG, nterms=8)                                                            # 72 > 64
    assert not refused(K.conv_tap_form, **dict(BIG, taps=[(0, 0, 0)]), nterms=8)
    assert refused(K.conv_tap_form, **dict(BIG, taps=[(0, 0, 0)]), nterms=9)
    assert refused(K.conv_tap_form, **dict(BIG, Cout=64), nterms=3) and refused(K.conv_tap_form, **dict(BIG, Cin=96), nterms=3)
    assert refused(K.conv_tap_form, **BIG, nterms=3, variant=K.CONV_STREAM256) and refused(K.conv_tap_form, **BIG, nterms=3, accumulate=True)
    assert refused(K.conv_tap_form, **BIG, nterms=3, head_c4=16)


# ------------------------------------------------------------------ LOFT_CONV_AUTO

# One convolution R x R, stride 1, pad R // 2 on a B x H x W map (M = B * H * W rows, Kdim = R * R * Cin) per row, and what the
# dispatcher takes for it under stream form 0.  EXPECTED VALUES BY HAND from the rule (include/loft_hip.h; fills(m, n) =
# ceil(M / m) * (Cout / n) * groups >= 192 workgroups):
#   64 -> 64 channels, 4..9 taps within -1..1, same-size bf16 map, M >= 65536            -> PATCH64
#   Cout % 256 == 0, bf16 out: !fills(256,256), fills(128,256), Kdim >= 1024              -> STREAM128
#                              !fills(128,256), fills(64,256),  Kdim >= 2048              -> STREAM64
#                              !fills(64,256),  fills(64,128),  Kdim >= 2048              -> STREAM64N
#                              fills(256,256)                                             -> STREAM256
#   Cout % 256 == 0, fills(256,256), Kdim >= 512 (fp32 / accumulating)                    -> T256_FAST if Kdim >= 1024 else T256
#   Cout % 128 == 0, bf16 out, Kdim >= 1024, fills(256,128)                               -> STREAM256 (128-cout tiles when Cout % 256)
#   Cout % 128 == 0: Kdim <= 512, LDS-staged output (not accumulating), not residual + mask of a dense 16-bit output -> T128_SINGLE
#                    else                                                                 -> T128_FAST if Kdim >= 1024 else T128
#   else                                                                                  -> T128x64
# (id, G, B, H, W, Cin, Cout, R, extra query arguments, kernel, tile pixels, tile couts)
AUTO_ROWS = [
    # fills(256,256): 192 x 256-pixel tiles; M = 191 * 256 + 1 | 191 * 256
    ('fill256_at', 1, 1, 27, 1811, 1024, 256, 1, {}, 'STREAM256', 256, 256),
    ('fill256_below', 1, 1, 191, 256, 1024, 256, 1, {}, 'STREAM128', 128, 256),
    ('fill256_at_shallow', 1, 1, 27, 1811, 64, 256, 1, {}, 'STREAM256', 256, 256),          # (no K-depth condition on the 256 tile)
    ('fill256_below_shallow', 1, 1, 191, 256, 64, 256, 1, {}, 'T128_SINGLE', 128, 128),
    ('fill256_groups4_at', 4, 1, 9, 1337, 1024, 256, 1, {}, 'STREAM256', 256, 256),         # 48 tiles x 4 groups
    ('fill256_groups4_below', 4, 1, 47, 256, 1024, 256, 1, {}, 'STREAM128', 128, 256),
    ('fill256_cout512_at', 1, 1, 95, 256 + 1, 1024, 512, 1, {}, 'STREAM256', 256, 256),     # M = 24415: 96 tiles x 2 channel tiles
    ('fill256_cout512_below', 1, 1, 95, 256, 1024, 512, 1, {}, 'STREAM128', 128, 256),
    # STREAM128: Kdim >= 1024
    ('stream128_kdim_960', 1, 1, 191, 256, 960, 256, 1, {}, 'T128', 128, 128),
    # fills(128,256): M = 191 * 128 + 1 | 191 * 128
    ('fill128_at', 1, 1, 23, 1063, 2048, 256, 1, {}, 'STREAM128', 128, 256),
    ('fill128_below', 1, 1, 191, 128, 2048, 256, 1, {}, 'STREAM64', 64, 256),
    # STREAM64: Kdim >= 2048 (8 x 32 x 32 rows, Cout 512: 64 / 128 / 256 workgroups on 256- / 128- / 64-pixel tiles)
    ('stream64_kdim_2048', 1, 8, 32, 32, 2048, 512, 1, {}, 'STREAM64', 64, 256),
    ('stream64_kdim_1984', 1, 8, 32, 32, 1984, 512, 1, {}, 'T128_FAST', 128, 128),
    # fills(64,256): M = 191 * 64 + 1 | 191 * 64
    ('fill64_at', 1, 1, 75, 163, 2048, 256, 1, {}, 'STREAM64', 64, 256),
    ('fill64_below', 1, 1, 191, 64, 2048, 256, 1, {}, 'STREAM64N', 64, 128),
    # fills(64,128): 96 x 64-pixel tiles x 2 cout tiles; M = 95 * 64 + 1 | 95 * 64; STREAM64N: Kdim >= 2048
    ('fill64n_at', 1, 1, 3, 2027, 2048, 256, 1, {}, 'STREAM64N', 64, 128),
    ('fill64n_below', 1, 1, 95, 64, 2048, 256, 1, {}, 'T128_FAST', 128, 128),
    ('stream64n_kdim_1984', 1, 1, 3, 2027, 1984, 256, 1, {}, 'T128_FAST', 128, 128),
    # fp32 / accumulating launches keep the lockstep kernels: T256 needs fills(256,256) and Kdim >= 512, FAST Kdim >= 1024
    ('f32_t256_fast', 1, 1, 27, 1811, 1024, 256, 1, dict(out_f32=True), 'T256_FAST', 256, 256),
    ('f32_t256_kdim_960', 1, 1, 27, 1811, 960, 256, 1, dict(out_f32=True), 'T256', 256, 256),
    ('f32_t256_kdim_512', 1, 1, 27, 1811, 512, 256, 1, dict(out_f32=True), 'T256', 256, 256),
    ('f32_t256_kdim_448', 1, 1, 27, 1811, 448, 256, 1, dict(out_f32=True), 'T128_SINGLE', 128, 128),
    ('f32_acc_kdim_448', 1, 1, 27, 1811, 448, 256, 1, dict(out_f32=True, accumulate=True), 'T128', 128, 128),     # (no staged output)
    ('f32_acc_t256', 1, 1, 27, 1811, 512, 256, 1, dict(out_f32=True, accumulate=True), 'T256', 256, 256),
    ('f32_below_fill256', 1, 1, 191, 256, 1024, 256, 1, dict(out_f32=True), 'T128_FAST', 128, 128),
    ('f32_at_fill128', 1, 1, 23, 1063, 2048, 256, 1, dict(out_f32=True), 'T128_FAST', 128, 128),
    # Cout % 256 / % 128 / % 4.  Cout = 384: fills(256,128) = 64 pixel tiles x 3; M = 63 * 256 + 1 | 63 * 256
    ('cout384_at', 1, 1, 127, 127, 1024, 384, 1, {}, 'STREAM256', 256, 128),
    ('cout384_below', 1, 1, 63, 256, 1024, 384, 1, {}, 'T128_FAST', 128, 128),
    ('cout384_kdim_960', 1, 1, 127, 127, 960, 384, 1, {}, 'T128', 128, 128),
    ('cout384_f32', 1, 1, 127, 127, 1024, 384, 1, dict(out_f32=True), 'T128_FAST', 128, 128),
    ('cout192', 1, 1, 127, 127, 1024, 192, 1, {}, 'T128x64', 128, 64),
    ('cout64_deep', 1, 8, 64, 64, 1024, 64, 1, {}, 'T128x64', 128, 64),
    # T128_SINGLE: Kdim <= 512, not the residual + mask of a dense 16-bit output
    ('single_kdim_512', 1, 2, 17, 19, 512, 128, 1, {}, 'T128_SINGLE', 128, 128),
    ('single_kdim_576', 1, 2, 17, 19, 64, 128, 3, {}, 'T128', 128, 128),
    ('single_res_only', 1, 2, 17, 19, 512, 128, 1, dict(residual=True), 'T128_SINGLE', 128, 128),
    ('single_res_mask', 1, 2, 17, 19, 512, 128, 1, dict(residual=True, mask=True), 'T128', 128, 128),
    ('single_res_mask_f32', 1, 2, 17, 19, 512, 128, 1, dict(residual=True, mask=True, out_f32=True), 'T128_SINGLE', 128, 128),
    ('single_res_mask_strided_out', 1, 2, 17, 19, 512, 128, 1, dict(residual=True, mask=True, os=2), 'T128_SINGLE', 128, 128),
    ('single_no_staged_out', 1, 2, 17, 19, 512, 128, 1, dict(variant=K.CONV_AUTO | K.CONV_FLAG_NO_STAGED_OUT), 'T128', 128, 128),
    # the patch kernel: M >= 65536, 64 -> 64 channels, 4..9 taps within -1..1, bf16 output
    ('patch_at', 1, 1, 256, 256, 64, 64, 3, {}, 'PATCH64', 256, 64),
    ('patch_below', 1, 1, 255, 257, 64, 64, 3, {}, 'T128x64', 128, 64),
    ('patch_one_tap', 1, 1, 256, 256, 64, 64, 1, {}, 'T128x64', 128, 64),
    ('patch_dilated', 1, 1, 256, 256, 64, 64, 3, dict(dilation=2), 'T128x64', 128, 64),
    ('patch_f32', 1, 1, 256, 256, 64, 64, 3, dict(out_f32=True), 'T128x64', 128, 64),
    ('patch_groups2', 2, 1, 256, 256, 64, 64, 3, {}, 'T128x64', 128, 64),
    ('patch_cin128', 1, 1, 256, 256, 128, 64, 3, {}, 'T128x64', 128, 64),
]

# the headline conv_tap shapes of profiles/round6_bench_shapes.txt (G, B, OH, OW, Cin, Cout, T, ss, os), queried only, with the
# kernel the shipped stream form (2) launches for them and whether their rows are pixel-major
BENCH_ROWS = [
    ((4, 2048, 7, 7, 256, 256, 9, 1, 1), 'LEAN', 256, 256, True),
    ((1, 2048, 14, 14, 256, 256, 9, 1, 1), 'LEAN', 256, 256, True),
    ((1, 8, 256, 256, 256, 256, 9, 1, 1), 'LEAN', 256, 256, False),
    ((1, 8, 128, 128, 128, 512, 1, 1, 1), 'LEAN', 256, 256, False),
    ((1, 2048, 14, 14, 256, 256, 1, 1, 2), 'LEAN', 256, 256, False),       # a parity launch of the 2x2 deconvolution
    ((1, 8, 64, 64, 256, 1024, 1, 1, 1), 'LEAN', 256, 256, False),
    ((1, 8, 64, 64, 256, 256, 9, 1, 1), 'STREAM128', 128, 256, False),
    ((1, 8192, 1, 1, 1024, 12544, 1, 1, 1), 'LEAN', 256, 256, False),
    ((1, 8, 256, 256, 64, 256, 9, 1, 1), 'LEAN', 256, 256, False),
    ((1, 8, 128, 128, 256, 256, 9, 1, 1), 'LEAN', 256, 256, False),
    ((1, 8192, 1, 1, 12544, 1024, 1, 1, 1), 'STREAM128', 128, 256, False),
    ((1, 8, 64, 64, 1024, 256, 1, 1, 1), 'STREAM128', 128, 256, False),
    ((1, 8, 128, 128, 128, 128, 9, 1, 1), 'STREAM256', 256, 128, False),
    ((1, 8, 128, 128, 512, 128, 1, 1, 1), 'T128_SINGLE', 128, 128, False),
    ((1, 8, 32, 32, 512, 512, 9, 1, 1), 'STREAM64', 64, 256, False),
    ((1, 8, 32, 32, 512, 2048, 1, 1, 1), 'LEAN', 256, 256, False),
    ((1, 8, 256, 256, 256, 64, 1, 1, 1), 'T128x64', 128, 64, False),
    ((1, 8, 32, 32, 256, 256, 9, 1, 1), 'STREAM64N', 64, 128, False),
]


def auto_query(row, lib_query=None):
    _, G, B, H, W, Cin, Cout, R, extra, _, _, _ = row
    extra = dict(extra)
    d, os_ = extra.pop('dilation', 1), extra.pop('os', 1)
    taps = [((r - R // 2) * d, (s - R // 2) * d, r * R + s) for r in range(R) for s in range(R)]
    return (lib_query or K.conv_tap_form)(B, H, W, Cin, Cout, H, W, H * os_, W * os_, taps, os=os_, groups=G, **extra)


def bench_query(shape):
    G, B, OH, OW, Cin, Cout, T, ss, os_ = shape
    taps = {9: [(r - 1, s - 1, r * 3 + s) for r in range(3) for s in range(3)], 1: [(0, 0, 0)]}[T]
    return K.conv_tap_form(B, OH * ss, OW * ss, Cin, Cout, OH, OW, OH * os_, OW * os_, taps, ss=ss, os=os_, groups=G)


def test_auto_table_has_both_sides_of_every_threshold():
    ids = [r[0] for r in AUTO_ROWS]
    assert len(set(ids)) == len(ids)
    for stem in ('fill256', 'fill256_groups4', 'fill256_cout512', 'fill128', 'fill64', 'fill64n', 'cout384', 'patch'):
        assert stem + '_at' in ids and stem + '_below' in ids, stem
    rows = {r[0]: r for r in AUTO_ROWS}
    m = lambda i: rows[i][1] * rows[i][2] * rows[i][3] * rows[i][4] // rows[i][1]        # rows of one group: B * H * W
    assert (m('fill256_at'), m('fill256_below')) == (191 * 256 + 1, 191 * 256) and (m('fill128_at'), m('fill128_below')) == (191 * 128 + 1, 191 * 128)
    assert (m('fill64_at'), m('fill64_below')) == (191 * 64 + 1, 191 * 64) and (m('fill64n_at'), m('fill64n_below')) == (95 * 64 + 1, 95 * 64)
    assert (m('fill256_groups4_at'), m('fill256_groups4_below')) == (47 * 256 + 1, 47 * 256)
    assert (m('fill256_cout512_at'), m('fill256_cout512_below')) == (95 * 257, 95 * 256) and -(-95 * 257 // 256) == 96
    assert (m('cout384_at'), m('cout384_below')) == (63 * 256 + 1, 63 * 256) and (m('patch_at'), m('patch_below')) == (65536, 65535)
    assert {r[9] for r in AUTO_ROWS} == set(KERNELS) - {'AUTO', 'PIPE256', 'ROLES256', 'STREAM256N', 'RING32', 'W4', 'XFIRST', 'LEAN', 'LEANX'}


@pytest.mark.parametrize('row', AUTO_ROWS, ids=[r[0] for r in AUTO_ROWS])
def test_auto_shape_reaches_its_kernel(row):
    with stream_form(0):
        f = auto_query(row)
    assert (name_of(f.kernel), f.tile_pixels, f.tile_couts) == row[9:], (row[0], f)


@pytest.mark.parametrize('row', BENCH_ROWS, ids=['x'.join(map(str, r[0])) for r in BENCH_ROWS])
def test_bench_shape_reaches_its_kernel(row):
    shape, kernel, tm, tn, pixmajor = row
    with stream_form(2):
        f = bench_query(shape)
    assert (name_of(f.kernel), f.tile_pixels, f.tile_couts, f.pixmajor) == (kernel, tm, tn, pixmajor), (shape, f)
    G, B, OH, OW = shape[:4]
    assert f.rows == B * OH * OW                         # 2048 RoIs: eight blocks of exactly 256, no padding rows


def test_both_builds_choose_the_same_kernel():
    """The bfloat16 and the binary16 build compile the same dispatcher."""
    prev = L.set_act16(torch.float16)
    try:
        with stream_form(0):
            f16 = [auto_query(r) for r in AUTO_ROWS]
    finally:
        L.set_act16(prev)
    assert [(name_of(f.kernel), f.tile_pixels, f.tile_couts) for f in f16] == [r[9:] for r in AUTO_ROWS]


# ------------------------------------------------------------------ pixel-major rows

@pytest.mark.parametrize('gid', ROI_GEOS)
def test_roi_geometries_are_pixel_major_in_blocks(gid):
    """The flag and the padded row count test_geometries_reach_their_hazards computes: max(1, B // 256) blocks of ceil(B / blocks)
    RoIs per position.  Off under NO_PIXMAJOR, one block under NO_ROI_BLOCKS; the lockstep FAST 256 tile has the mode without
    blocks, the other lockstep kernels do not have it."""
    geo = GEO[gid]
    la, P = geo.launches[0], geo.OHf * geo.OWf
    nb = max(1, geo.B // 256)
    S = -(-geo.B // nb)
    for k in PIPELINED:
        f = query(geo, la, EPI['bias_relu'], code(k))
        assert (f.pixmajor, f.rows) == (True, nb * P * S), (k, f)
        f = query(geo, la, EPI['bias_relu'], code(k) | K.CONV_FLAG_NO_PIXMAJOR)
        assert (f.pixmajor, f.rows) == (False, P * geo.B), (k, f)
        f = query(geo, la, EPI['bias_relu'], code(k) | K.CONV_FLAG_NO_ROI_BLOCKS)
        assert (f.pixmajor, f.rows) == (True, P * geo.B), (k, f)
    for k in LOCKSTEP:
        f = query(geo, la, EPI['bias_relu'], code(k))
        assert (f.pixmajor, f.rows) == (k == 'T256_FAST', P * geo.B), (k, f)
        assert not query(geo, la, EPI['bias_relu'], code(k) | K.CONV_FLAG_NO_PIXMAJOR).pixmajor
    f = query(geo, la, EPI['plain'], nterms=3)           # a plane launch: the same rows
    assert (f.pixmajor, f.rows) == (True, nb * P * S)


def test_pixel_major_needs_an_roi_map():
    """B >= 256, a map of <= 1024 pixels, more than one tap, unit strides, a dense output."""
    base = dict(B=256, IH=32, IW=32, Cin=64, Cout=256, OH=32, OW=32, OHf=32, OWf=32, variant=K.CONV_STREAM256,
                taps=[(r - 1, s - 1, r * 3 + s) for r in range(3) for s in range(3)])
    assert K.conv_tap_form(**base).pixmajor
    assert not K.conv_tap_form(**dict(base, B=255)).pixmajor
    assert not K.conv_tap_form(**dict(base, IW=33, OW=33, OWf=33)).pixmajor
    assert not K.conv_tap_form(**dict(base, taps=[(0, 0, 0)])).pixmajor
    assert not K.conv_tap_form(**dict(base, IH=64, IW=64), ss=2).pixmajor
    assert not K.conv_tap_form(**dict(base, OHf=64, OWf=64), os=2).pixmajor


# ------------------------------------------------------------------ stream forms

def test_stream256_reports_the_instance_of_the_stream_form():
    """Pinned or chosen, the 256 x 256 tile of STREAM256 launches XFIRST / LEAN / LEANX under forms 1 / 2 / 3 (bit 2 is the plane
    launches' epilogue: no other instance); a tap-major launch under form 2 or 3 falls back to form 0."""
    geo = GEO['fwd3x3_ragged']
    la = geo.launches[0]
    for form, want, want_tm in ((0, 'STREAM256', 'STREAM256'), (1, 'XFIRST', 'XFIRST'), (2, 'LEAN', 'STREAM256'), (3, 'LEANX', 'STREAM256'),
                                (6, 'LEAN', 'STREAM256')):
        with stream_form(form):
            assert name_of(query(geo, la, EPI['bias_relu'], K.CONV_STREAM256).kernel) == want, form
            assert name_of(K.conv_tap_form(**BIG).kernel) == want, form
            assert name_of(query(geo, la, EPI['bias_relu'], K.CONV_STREAM256 | K.CONV_FLAG_TAP_MAJOR).kernel) == want_tm, form
            assert name_of(K.conv_tap_form(**BIG, variant=K.CONV_AUTO | K.CONV_FLAG_TAP_MAJOR).kernel) == want_tm, form
            assert name_of(query(geo, la, EPI['bias_relu'], K.CONV_STREAM256 | K.CONV_FLAG_KROT).kernel) == want, form
            # what has no forms: the experiment instances, the 128-cout tiles, every other code
            assert name_of(query(geo, la, EPI['bias_relu'], K.CONV_STREAM256 | (2 << 12)).kernel) == 'STREAM256'
            n128 = GEO['fwd3x3_s2_n128']
            f = query(n128, n128.launches[0], EPI['bias_relu'], K.CONV_STREAM256)
            assert (name_of(f.kernel), f.tile_couts) == ('STREAM256', 128)
            for k in ('PIPE256', 'STREAM128', 'STREAM64', 'STREAM64N', 'ROLES256', 'STREAM256N', 'RING32', 'W4', 'XFIRST', 'LEAN', 'LEANX'):
                assert name_of(query(geo, la, EPI['bias_relu'], code(k)).kernel) == k, (form, k)


def test_plane_launches_take_the_largest_stream_tile_that_fills_the_chip():
    """... and LEAN only for forms >= 2 on the 256 x 256 tile.  The tile rule of the plane launches: fills(256,256) -> 256 x 256,
    fills(128,256) -> 128 x 256, fills(64,256) -> 64 x 256, else 64 x 128, with no K-depth condition; Cout % 256: 256 x 128 where
    that fills the chip, else 64 x 128."""
    for form, want in ((0, 'STREAM256'), (1, 'STREAM256'), (2, 'LEAN'), (3, 'LEAN'), (6, 'LEAN')):
        with stream_form(form):
            f = K.conv_tap_form(**BIG, nterms=3)
            assert (name_of(f.kernel), f.tile_pixels, f.tile_couts) == (want, 256, 256), form
            for shape, tile in (((1, 1, 191, 256, 64, 256), ('STREAM128', 128, 256)),             # 191 x 256-pixel tiles, K shallow
                                ((1, 1, 191, 128, 64, 256), ('STREAM64', 64, 256)),
                                ((1, 1, 191, 64, 64, 256), ('STREAM64N', 64, 128)),
                                ((1, 2, 17, 19, 64, 256), ('STREAM64N', 64, 128)),               # fills nothing: stays on the smallest
                                ((1, 1, 127, 127, 64, 384), ('STREAM256', 256, 128)),
                                ((1, 1, 63, 256, 64, 384), ('STREAM64N', 64, 128)),
                                ((1, 2, 17, 19, 64, 128), ('STREAM64N', 64, 128))):
                G, B, H, W, Cin, Cout = shape
                f = K.conv_tap_form(B, H, W, Cin, Cout, H, W, H, W, [(0, 0, 0)], groups=G, nterms=3)
                assert (name_of(f.kernel), f.tile_pixels, f.tile_couts) == tile, (form, shape, f)
