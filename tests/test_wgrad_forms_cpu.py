"""CPU: which kernel the 16-bit weight-gradient dispatcher takes for a shape (loft_conv_wgrad_form, a host-only query of the
launch path itself).  FORMS / DECONV_FORMS hold one small, ragged shape (and more) for every kernel of the family, each with the
form it was written for -- the table tests/test_wgrad_forms_gpu.py is parametrised over: moving a dispatch threshold fails here,
without a GPU, instead of silently leaving that file's cases on another kernel."""
import os

import pytest
import torch  # noqa: F401  (load torch's HIP runtime before libloft_hip.so)

from bonai_amd import kernels as K
from bonai_amd import lib as L

# (id, groups, B, Cin, Cout, H, W, R, stride, pad, variant, splits, expected form); variant / form: the K.WGRAD_* / K.WGRAD_FORM_* names
FORMS = [
    # lockstep 128 x 128 tile
    ('t128_3x3', 1, 2, 128, 256, 17, 19, 3, 1, 1, 'T128', 0, 'T128'),
    ('t128_3x3_s2', 1, 2, 256, 128, 17, 17, 3, 2, 1, 'T128', 0, 'T128'),
    ('t128_1x1_s2', 1, 2, 256, 128, 16, 16, 1, 2, 0, 'T128', 0, 'T128'),
    ('t128_pm', 1, 130, 128, 128, 5, 9, 3, 1, 1, 'T128', 0, 'T128_PM'),
    ('t128_pm_splits5', 1, 130, 128, 128, 5, 9, 3, 1, 1, 'T128', 5, 'T128_PM'),
    # lockstep 256 x 256 tile
    ('t256_3x3', 1, 1, 256, 256, 17, 19, 3, 1, 1, 'T256', 0, 'T256'),
    ('t256_3x3_splits3', 1, 1, 256, 256, 17, 19, 3, 1, 1, 'T256', 3, 'T256'),
    ('t256_1x1', 1, 3, 256, 512, 9, 11, 1, 1, 0, 'T256', 0, 'T256'),
    ('t256_pm', 1, 130, 256, 256, 5, 9, 3, 1, 1, 'T256', 0, 'T256_PM'),
    ('t256_pm_groups4', 4, 130, 256, 256, 7, 7, 3, 1, 1, 'T256', 0, 'T256_PM'),
    # four-stage ring, 128 x 128 tile
    ('ring_generic', 1, 2, 128, 256, 17, 19, 3, 1, 1, 'RING128', 0, 'RING_GENERIC'),
    ('ring_generic_s2', 1, 2, 256, 128, 17, 17, 3, 2, 1, 'RING128', 0, 'RING_GENERIC'),
    ('ring_dense', 1, 3, 128, 384, 9, 11, 1, 1, 0, 'RING128', 0, 'RING_DENSE'),
    ('ring_same', 1, 1, 128, 128, 3, 35, 3, 1, 1, 'RING128', 0, 'RING_SAME'),
    ('ring_same_m255', 1, 1, 128, 128, 5, 51, 3, 1, 1, 'RING128', 0, 'RING_SAME'),
    ('ring_same_m255_splits2', 1, 1, 128, 128, 5, 51, 3, 1, 1, 'RING128', 2, 'RING_SAME'),
    ('ring_same_m129', 1, 1, 128, 128, 3, 43, 3, 1, 1, 'RING128', 0, 'RING_SAME'),
    ('ring_same_m129_splits2', 1, 1, 128, 128, 3, 43, 3, 1, 1, 'RING128', 2, 'RING_SAME'),
    # software-pipelined stream, 256 x 256 tile
    ('stream_generic', 1, 1, 256, 256, 17, 19, 3, 1, 1, 'STREAM256', 0, 'STREAM_GENERIC'),
    ('stream_generic_splits3', 1, 1, 256, 256, 17, 19, 3, 1, 1, 'STREAM256', 3, 'STREAM_GENERIC'),
    ('stream_generic_s2', 1, 2, 256, 256, 17, 17, 3, 2, 1, 'STREAM256', 0, 'STREAM_GENERIC'),
    ('stream_dense', 1, 3, 256, 512, 9, 11, 1, 1, 0, 'STREAM256', 0, 'STREAM_DENSE'),
    ('stream_same', 1, 1, 256, 256, 5, 67, 3, 1, 1, 'STREAM256', 0, 'STREAM_SAME'),
    ('stream_pm_inc', 1, 130, 256, 256, 5, 9, 3, 1, 1, 'STREAM256', 1, 'STREAM_PM_INC'),
    ('stream_pm_inc_64_rois_per_split', 1, 128, 256, 256, 5, 9, 3, 1, 1, 'STREAM256', 2, 'STREAM_PM_INC'),
    ('stream_pm', 1, 130, 256, 256, 5, 9, 3, 1, 1, 'STREAM256', 0, 'STREAM_PM'),
    ('stream_pm_splits5', 1, 130, 256, 256, 5, 9, 3, 1, 1, 'STREAM256', 5, 'STREAM_PM'),
    ('stream_pm_groups4', 4, 130, 256, 256, 7, 7, 3, 1, 1, 'STREAM256', 0, 'STREAM_PM'),
    # 64-channel narrow kernel
    ('narrow_generic', 1, 2, 24, 40, 9, 11, 3, 1, 1, 'AUTO', 0, 'NARROW_GENERIC'),
    ('narrow_generic_s2', 1, 2, 64, 48, 9, 11, 3, 2, 1, 'AUTO', 0, 'NARROW_GENERIC'),
    ('narrow_dense', 1, 3, 64, 192, 9, 11, 1, 1, 0, 'AUTO', 0, 'NARROW_DENSE'),
    ('narrow_same', 1, 1, 32, 64, 3, 67, 3, 1, 1, 'AUTO', 0, 'NARROW_SAME'),
    # a single, partial K-step (M = 15 pixels)
    ('one_kstep_c128_t128', 1, 1, 128, 128, 3, 5, 3, 1, 1, 'T128', 0, 'T128'),
    ('one_kstep_c128_ring', 1, 1, 128, 128, 3, 5, 3, 1, 1, 'RING128', 0, 'RING_GENERIC'),
    ('one_kstep_c256_t128', 1, 1, 256, 256, 3, 5, 3, 1, 1, 'T128', 0, 'T128'),
    ('one_kstep_c256_ring', 1, 1, 256, 256, 3, 5, 3, 1, 1, 'RING128', 0, 'RING_GENERIC'),
    ('one_kstep_c256_t256', 1, 1, 256, 256, 3, 5, 3, 1, 1, 'T256', 0, 'T256'),
    ('one_kstep_c256_stream', 1, 1, 256, 256, 3, 5, 3, 1, 1, 'STREAM256', 0, 'STREAM_GENERIC'),
]

# the transposed convolution 2x2 / stride 2 (nn._DeconvFn.backward): G is the [N, 2H, 2W, Cout] output gradient, X the [N, H, W, Cin]
# input, taps (py, px, 0, 0, 2 py + px) with gos = 2, the bias gradient from every tap (db_tap = -2)
# (id, N, H, W, Cin, Cout, variant, splits, expected form)
DECONV_FORMS = [
    ('deconv_c256_stream', 3, 7, 5, 256, 256, 'STREAM256', 0, 'STREAM_GENERIC'),
    ('deconv_c256_t256', 3, 7, 5, 256, 256, 'T256', 0, 'T256'),
    ('deconv_c256_ring', 3, 7, 5, 256, 256, 'RING128', 0, 'RING_GENERIC'),
    ('deconv_c256_t128', 3, 7, 5, 256, 256, 'T128', 0, 'T128'),
    ('deconv_c128_ring', 3, 7, 5, 128, 128, 'RING128', 0, 'RING_GENERIC'),
    ('deconv_c128_t128', 3, 7, 5, 128, 128, 'T128', 0, 'T128'),
]

# the thresholds of the dispatcher under WGRAD_AUTO, one shape on either side (queried only: some of these are too large to run in a test)
THRESHOLDS = [
    # M * (Cout / 256) * (Cin / 256) * T * groups >= 524288 -> the 256 x 256 stream kernel
    ('auto_work_at_threshold', 4, 298, 256, 256, 7, 7, 3, 1, 1, 'AUTO', 0, 'STREAM_PM'),
    ('auto_work_below_threshold', 4, 297, 256, 256, 7, 7, 3, 1, 1, 'AUTO', 0, 'T128_PM'),
    ('auto_1x1_work_at_threshold', 1, 8, 256, 256, 256, 256, 1, 1, 0, 'AUTO', 0, 'STREAM_DENSE'),
    ('auto_1x1_work_below_threshold', 1, 8, 256, 256, 256, 255, 1, 1, 0, 'AUTO', 0, 'RING_DENSE'),
    # same-size row addressing: OW >= 32 (ring), OW >= 64 (stream, narrow)
    ('ring_same_w32', 1, 1, 128, 128, 3, 32, 3, 1, 1, 'AUTO', 0, 'RING_SAME'),
    ('ring_same_w31', 1, 1, 128, 128, 3, 31, 3, 1, 1, 'AUTO', 0, 'RING_GENERIC'),
    ('stream_same_w64', 1, 1, 256, 256, 3, 64, 3, 1, 1, 'STREAM256', 0, 'STREAM_SAME'),
    ('stream_same_w63', 1, 1, 256, 256, 3, 63, 3, 1, 1, 'STREAM256', 0, 'STREAM_GENERIC'),
    ('narrow_same_w64', 1, 1, 32, 64, 3, 64, 3, 1, 1, 'AUTO', 0, 'NARROW_SAME'),
    ('narrow_same_w63', 1, 1, 32, 64, 3, 63, 3, 1, 1, 'AUTO', 0, 'NARROW_GENERIC'),
    # valid-rows form: B >= 128, OH * OW <= 1024, more than one tap, unit strides
    ('pm_b128', 1, 128, 128, 128, 5, 9, 3, 1, 1, 'T128', 0, 'T128_PM'),
    ('pm_b127', 1, 127, 128, 128, 5, 9, 3, 1, 1, 'T128', 0, 'T128'),
    ('pm_map_1024', 1, 128, 128, 128, 32, 32, 3, 1, 1, 'T128', 0, 'T128_PM'),
    ('pm_map_1056', 1, 128, 128, 128, 32, 33, 3, 1, 1, 'T128', 0, 'T128'),
    ('pm_one_tap', 1, 130, 128, 128, 5, 9, 1, 1, 0, 'T128', 0, 'T128'),
    ('pm_stride2', 1, 130, 128, 128, 9, 9, 3, 2, 1, 'T128', 0, 'T128'),
    # incremental addressing of the stream valid-rows form: every tap's split holds >= 64 RoIs
    ('stream_pm_b128_3splits', 1, 128, 256, 256, 5, 9, 3, 1, 1, 'STREAM256', 3, 'STREAM_PM'),
]

ALL_FORMS = ['T128', 'T128_PM', 'T256', 'T256_PM', 'RING_GENERIC', 'RING_DENSE', 'RING_SAME', 'STREAM_GENERIC', 'STREAM_PM_INC',
             'STREAM_DENSE', 'STREAM_SAME', 'STREAM_PM', 'NARROW_GENERIC', 'NARROW_DENSE', 'NARROW_SAME']


def conv_geometry(row):
    """A FORMS row -> the arguments of K.conv_wgrad / K.conv_wgrad_form for that convolution (what K.conv2d_wgrad passes)."""
    _, G, B, Cin, Cout, H, W, R, stride, pad, variant, splits, _ = row
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    taps = [(0, 0, r - pad, s - pad, r * R + s) for r in range(R) for s in range(R)]
    return dict(B=B, GH=OH, GW=OW, Cout=Cout, XH=H, XW=W, Cin=Cin, OH=OH, OW=OW, taps=taps, gos=1, ss=stride, groups=G, splits=splits,
                variant=getattr(K, 'WGRAD_' + variant))


def deconv_geometry(row):
    _, N, H, W, Cin, Cout, variant, splits, _ = row
    taps = [(py, px, 0, 0, py * 2 + px) for py in range(2) for px in range(2)]
    return dict(B=N, GH=2 * H, GW=2 * W, Cout=Cout, XH=H, XW=W, Cin=Cin, OH=H, OW=W, taps=taps, gos=2, ss=1, groups=1, splits=splits,
                variant=getattr(K, 'WGRAD_' + variant))


def expected_form(row):
    return getattr(K, 'WGRAD_FORM_' + row[-1])


def form_name(code):
    names = [n for n in ALL_FORMS if getattr(K, 'WGRAD_FORM_' + n) == code]
    return names[0] if names else code


@pytest.fixture(scope='module', autouse=True)
def _library():
    if not (os.path.exists(L._LIB_PATH) and os.path.exists(L._LIB_PATH_F16)):
        from bonai_amd import build
        build.build()


def test_form_codes_are_distinct():
    codes = [getattr(K, 'WGRAD_FORM_' + n) for n in ALL_FORMS]
    assert len(set(codes)) == 15 and K.WGRAD_FORM_NONE not in codes and all(c > 0 for c in codes)


@pytest.mark.parametrize('row', FORMS + THRESHOLDS, ids=[r[0] for r in FORMS + THRESHOLDS])
def test_conv_shape_reaches_its_form(row):
    got = K.conv_wgrad_form(**conv_geometry(row))
    assert got == expected_form(row), (row[0], form_name(got), row[-1])


@pytest.mark.parametrize('row', DECONV_FORMS, ids=[r[0] for r in DECONV_FORMS])
def test_deconv_shape_reaches_its_form(row):
    got = K.conv_wgrad_form(**deconv_geometry(row))
    assert got == expected_form(row), (row[0], form_name(got), row[-1])


def test_table_reaches_every_form():
    """FORMS / DECONV_FORMS cover all fifteen kernels of the family (the THRESHOLDS rows do not count: some are bench-sized)."""
    reached = {K.conv_wgrad_form(**conv_geometry(r)) for r in FORMS} | {K.conv_wgrad_form(**deconv_geometry(r)) for r in DECONV_FORMS}
    assert {r[-1] for r in FORMS} == set(ALL_FORMS)
    assert reached == {getattr(K, 'WGRAD_FORM_' + n) for n in ALL_FORMS}, sorted(form_name(c) for c in reached)


def test_both_builds_choose_the_same_form():
    """The bfloat16 and the binary16 build compile the same dispatcher."""
    prev = L.set_act16(torch.float16)
    try:
        f16 = [K.conv_wgrad_form(**conv_geometry(r)) for r in FORMS + THRESHOLDS]
    finally:
        L.set_act16(prev)
    assert f16 == [expected_form(r) for r in FORMS + THRESHOLDS]


def test_form_query_agrees_with_the_slots_query_on_what_is_launched():
    """No launch (no pixel, or no tap with a valid row) is WGRAD_FORM_NONE; arguments the launch rejects are rejected."""
    geo = conv_geometry(FORMS[0])
    assert K.conv_wgrad_form(**dict(geo, B=0)) == K.WGRAD_FORM_NONE
    far = [(0, 0, 40, 40, i) for i in range(9)]          # every tap leaves the 5 x 9 map: the valid-rows form has nothing to launch
    assert K.conv_wgrad_form(**dict(conv_geometry([r for r in FORMS if r[0] == 't128_pm'][0]), taps=far)) == K.WGRAD_FORM_NONE
    with pytest.raises(L.LoftHipError):
        K.conv_wgrad_form(**dict(geo, variant=K.WGRAD_STREAM256))         # Cin = 128: no 256 x 256 tile
    with pytest.raises(L.LoftHipError):
        K.conv_wgrad_form(**dict(conv_geometry([r for r in FORMS if r[0] == 'narrow_generic'][0]), variant=K.WGRAD_T128))     # narrow channels: no 128 x 128 tile
