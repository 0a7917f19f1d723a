"""CPU: the whole plan of a 16-bit weight-gradient launch (K.conv_wgrad_plan -> loft_conv_wgrad_plan, a host-only query of
wgrad_plan, the function the launches themselves call).  tests/test_wgrad_forms_cpu.py pins the FORM of its tables' shapes; here,
for the same tables and for the weight-gradient shapes of the bench step, without a GPU:
  - the plan query, the form query and the slot query answer alike, rejections included;
  - grid, block threads, split count, split length and the per-tap tables of the valid-rows (PM) form equal `restate` below: the
    dispatcher's rule as it stood BEFORE the plan existed (one function, wgrad_impl), written out again in Python from that code.
    PARENT_SLOTS / BENCH rows carry the slot counts that build returned from loft_conv_wgrad_slots, recorded as literals: they tie
    the restatement to the old code, the restatement ties the new code to it;
  - operand-plane launches count groups x terms virtual groups in grid.y, the split target and the work threshold;
  - the bfloat16 and the binary16 build answer identically."""
import ctypes
import os

import pytest
import torch  # noqa: F401  (load torch's HIP runtime before libloft_hip.so)

from bonai_amd import kernels as K
from bonai_amd import lib as L
from test_wgrad_forms_cpu import DECONV_FORMS, FORMS, THRESHOLDS, conv_geometry, deconv_geometry, form_name

ROWS = [(r[0], conv_geometry(r)) for r in FORMS + THRESHOLDS] + [(r[0], deconv_geometry(r)) for r in DECONV_FORMS]
IDS = [i for i, _ in ROWS]


@pytest.fixture(scope='module', autouse=True)
def _library():
    if not (os.path.exists(L._LIB_PATH) and os.path.exists(L._LIB_PATH_F16)):
        from bonai_amd import build
        build.build()


def cdiv(a, b):
    return -(-a // b)


def restate(B, GH, GW, Cout, XH, XW, Cin, OH, OW, taps, gos=1, ss=1, groups=1, splits=0, variant=K.WGRAD_AUTO, nterms=0):
    """What the dispatcher decided for an ACCEPTED launch before wgrad_plan: None when nothing is launched, else a dict."""
    T = len(taps)
    narrow = Cin % 128 != 0 or Cout % 128 != 0
    slots_ok = not narrow and sorted(t[4] for t in taps) == list(range(T))
    groups *= max(1, nterms)                                  # operand planes: virtual groups from here on
    M = B * OH * OW
    if M <= 0:
        return None
    if variant == K.WGRAD_AUTO:
        big = Cout % 256 == 0 and Cin % 256 == 0 and M * (Cout // 256) * (Cin // 256) * T * groups >= 524288
    else:
        big = variant not in (K.WGRAD_T128, K.WGRAD_RING128)
    tile = 64 if narrow else 256 if big else 128
    tiles = cdiv(Cout, tile) * cdiv(Cin, tile)
    if splits <= 0:
        ring = not narrow and variant != K.WGRAD_T128 and gos == 1 and ss == 1 and (GH, GW) == (OH, OW) == (XH, XW)
        want = (256 if big else 288 if ring else 512) // (tiles * T * groups)
        splits = max(1, min(want, cdiv(M, 256)))
    pps = cdiv(cdiv(M, splits), 64) * 64
    out = dict(tile=tile, threads=512 if big else 256, pix_per_split=pps)
    if not narrow and T > 1 and gos == 1 and ss == 1 and B >= 128 and OH * OW <= 1024:
        budget = min(splits * T, 256)
        npos = []
        for goy, gox, dy, dx, _ in taps:
            rh = min(OH, GH - goy, XH - dy) - max(0, -goy, -dy)
            rw = min(OW, GW - gox, XW - dx) - max(0, -gox, -dx)
            npos.append(max(0, rh) * max(0, rw))
        total = sum(npos) * B
        if total == 0:
            return None
        Lk = cdiv(cdiv(total, budget), 64) * 64               # rows per split, common to the taps
        while sum(cdiv(B, max(1, Lk // p)) for p in npos if p) > budget:
            Lk += 64
        ns = [cdiv(B, max(1, Lk // p)) if p else 0 for p in npos]
        return dict(out, pm=True, grid=(tiles, groups, sum(ns)), splits=splits, pm_splits=tuple(ns),
                    pm_pps=tuple(cdiv(B, n) if n else 1 for n in ns), nslots=max(ns) if slots_ok and all(ns) else 0)
    splits = cdiv(M, pps)
    return dict(out, pm=False, grid=(tiles, T * groups, splits), splits=splits, pm_splits=(), pm_pps=(), nslots=splits if slots_ok else 0)


def as_dict(p):
    return dict(tile=p.tile, threads=p.threads, pix_per_split=p.pix_per_split, pm=p.pm, grid=p.grid, splits=p.splits,
                pm_splits=p.pm_splits, pm_pps=p.pm_pps, nslots=p.nslots)


def slots_query(g):
    """loft_conv_wgrad_slots of the active build: the slot count, 0, or -hipError_t."""
    A = lambda i: L.arr(ctypes.c_int, [t[i] for t in g['taps']])
    return L.load().loft_conv_wgrad_slots(g['B'], g['GH'], g['GW'], g['Cout'], g['XH'], g['XW'], g['Cin'], g['OH'], g['OW'], g['gos'], g['ss'],
                                          len(g['taps']), A(0), A(1), A(2), A(3), A(4), g['groups'], g['splits'], int(g['variant']))


def refused(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except L.LoftHipError as e:
        assert 'hipError_t 1' in str(e), e              # hipErrorInvalidValue, nothing else
        return True
    return False


def test_plan_indices_are_the_header_s():
    """K.WGRAD_PLAN_* mirror every LOFT_WGRAD_PLAN_* of include/loft_hip.h; the two per-tap tables hold 16 entries each."""
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'loft_hip.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define\s+LOFT_(WGRAD_PLAN_[A-Z_]+)\s+(\d+)\b', hdr, re.M)}
    assert len(defs) == 13 and all(getattr(K, n) == v for n, v in defs.items()), defs
    assert K.WGRAD_PLAN_PM_PPS - K.WGRAD_PLAN_PM_NS == K.WGRAD_PLAN_LEN - K.WGRAD_PLAN_PM_PPS == 16


# ------------------------------------------------------------------ the three queries agree

@pytest.mark.parametrize('geo', [g for _, g in ROWS], ids=IDS)
def test_plan_form_and_slot_queries_agree(geo):
    p = K.conv_wgrad_plan(**geo)
    assert p.form == K.conv_wgrad_form(**geo) and p.form != K.WGRAD_FORM_NONE
    assert p.nslots == slots_query(geo)


def test_queries_agree_on_what_is_not_launched_and_what_is_rejected():
    geo = dict(ROWS)['t128_3x3']
    far = [(0, 0, 40, 40, i) for i in range(9)]          # every tap leaves the 5 x 9 map: the valid-rows form has nothing to launch
    for g in (dict(geo, B=0), dict(dict(ROWS)['t128_pm'], taps=far)):
        p = K.conv_wgrad_plan(**g)
        assert K.conv_wgrad_form(**g) == K.WGRAD_FORM_NONE and slots_query(g) == 0
        assert p == K.WgradPlan(K.WGRAD_FORM_NONE, 0, 0, (0, 0, 0), 0, 0, 0, False, (), ())
    narrow = dict(ROWS)['narrow_generic']
    for g in (dict(geo, variant=K.WGRAD_STREAM256), dict(narrow, variant=K.WGRAD_T128), dict(geo, variant=5), dict(geo, variant=-1),
              dict(geo, groups=0), dict(geo, Cin=100), dict(geo, taps=geo['taps'] * 2), dict(geo, B=1 << 21, OH=64, GH=64, XH=64)):           # (2^27 x 19 rows: more than 2^31 - 1)
        assert refused(K.conv_wgrad_plan, **g) and refused(K.conv_wgrad_form, **g) and slots_query(g) == -1, g
    # no pixel: no launch, whatever the variant (the variant is held against the channels only when there is one)
    assert K.conv_wgrad_plan(**dict(geo, B=0, variant=K.WGRAD_STREAM256)).form == K.WGRAD_FORM_NONE


def test_slot_count_is_zero_where_no_slot_launch_exists():
    """Narrow channels, a weight tap written twice or never, a valid-rows tap without a split: the plan is otherwise unchanged."""
    narrow = K.conv_wgrad_plan(**dict(ROWS)['narrow_same'])
    assert narrow.nslots == 0 and narrow.splits >= 1
    geo = dict(ROWS)['t128_3x3']
    twice = [t[:4] + (0 if i == 8 else t[4],) for i, t in enumerate(geo['taps'])]
    p, q = K.conv_wgrad_plan(**geo), K.conv_wgrad_plan(**dict(geo, taps=twice))
    assert p.nslots == p.splits > 1 and q == p._replace(nslots=0)
    pm = dict(ROWS)['t128_pm']
    one_out = [(0, 0, 40, 40, 0)] + pm['taps'][1:]
    p, q = K.conv_wgrad_plan(**pm), K.conv_wgrad_plan(**dict(pm, taps=one_out))
    assert p.nslots == max(p.pm_splits) >= 1 and q.pm and q.pm_splits[0] == 0 and all(q.pm_splits[1:]) and q.nslots == 0
    assert slots_query(dict(pm, taps=one_out)) == 0 and slots_query(dict(geo, taps=twice)) == 0


# ------------------------------------------------------------------ the plan against the rule it replaced

# loft_conv_wgrad_slots of the build BEFORE wgrad_plan, for every row of the three tables with wide channels
PARENT_SLOTS = {
    't128_3x3': 3, 't128_3x3_s2': 1, 't128_1x1_s2': 1, 't128_pm': 26, 't128_pm_splits5': 6, 't256_3x3': 2, 't256_3x3_splits3': 3,
    't256_1x1': 2, 't256_pm': 26, 't256_pm_groups4': 9, 'ring_generic': 3, 'ring_generic_s2': 1, 'ring_dense': 2, 'ring_same': 1,
    'ring_same_m255': 1, 'ring_same_m255_splits2': 2, 'ring_same_m129': 1, 'ring_same_m129_splits2': 2, 'stream_generic': 2,
    'stream_generic_splits3': 3, 'stream_generic_s2': 1, 'stream_dense': 2, 'stream_same': 2, 'stream_pm_inc': 1,
    'stream_pm_inc_64_rois_per_split': 2, 'stream_pm': 26, 'stream_pm_splits5': 6, 'stream_pm_groups4': 9,
    'one_kstep_c128_t128': 1, 'one_kstep_c128_ring': 1, 'one_kstep_c256_t128': 1, 'one_kstep_c256_ring': 1,
    'one_kstep_c256_t256': 1, 'one_kstep_c256_stream': 1, 'auto_work_at_threshold': 9, 'auto_work_below_threshold': 2,
    'auto_1x1_work_at_threshold': 256, 'auto_1x1_work_below_threshold': 72, 'ring_same_w32': 1, 'ring_same_w31': 1,
    'stream_same_w64': 1, 'stream_same_w63': 1, 'pm_b128': 26, 'pm_b127': 23, 'pm_map_1024': 32, 'pm_map_1056': 56,
    'pm_one_tap': 23, 'pm_stride2': 13, 'stream_pm_b128_3splits': 3, 'deconv_c256_stream': 1, 'deconv_c256_t256': 1,
    'deconv_c256_ring': 1, 'deconv_c256_t128': 1, 'deconv_c128_ring': 1, 'deconv_c128_t128': 1,
}


def test_restatement_is_the_rule_of_the_previous_build():
    wide = [i for i, g in ROWS if g['Cin'] % 128 == 0 and g['Cout'] % 128 == 0]
    assert sorted(PARENT_SLOTS) == sorted(wide) and len(wide) >= 50
    for i, g in ROWS:
        if i in PARENT_SLOTS:
            assert restate(**g)['nslots'] == PARENT_SLOTS[i], i
    assert all(v >= 1 for v in PARENT_SLOTS.values())


@pytest.mark.parametrize('geo', [g for _, g in ROWS], ids=IDS)
def test_plan_is_the_restated_rule(geo):
    assert as_dict(K.conv_wgrad_plan(**geo)) == restate(**geo)


def test_explicit_splits_budget_the_pm_blocks_and_are_recomputed_elsewhere():
    """splits > 0: the valid-rows form gets min(splits * T, 256) blocks per group and channel tile; every other form splits by the
    ROUNDED split length (M = 255 in two splits: 128 + 127 rows -> 128-row splits, two of them; in three: 85 -> 128, two again)."""
    pm = dict(ROWS)['t128_pm']
    for s in (1, 2, 5, 29, 40):
        p = K.conv_wgrad_plan(**dict(pm, splits=s))
        assert p.splits == s and p.grid[2] == sum(p.pm_splits) <= min(9 * s, 256) and as_dict(p) == restate(**dict(pm, splits=s)), s
    ring = dict(ROWS)['ring_same_m255']
    assert [K.conv_wgrad_plan(**dict(ring, splits=s)).splits for s in (1, 2, 3, 4)] == [1, 2, 2, 4]
    assert [K.conv_wgrad_plan(**dict(ring, splits=s)).pix_per_split for s in (1, 2, 3, 4)] == [256, 128, 128, 64]


# ------------------------------------------------------------------ the bench step

# The weight-gradient launches of the bench step (profiles/round6_bench_shapes.txt: groups, B, OH, OW, Cin, Cout, T, ss, gos), under
# WGRAD_AUTO with splits = 0, queried only -> the form by the rule of include/loft_hip.h, and loft_conv_wgrad_slots of the build
# before wgrad_plan.  T = 9: 3 x 3 / pad 1; T = 4, gos = 2: the 2 x 2 / stride-2 deconvolution; T = 1: 1 x 1 (8192 x 1 x 1: an FC).
BENCH = [
    ((4, 2048, 7, 7, 256, 256, 9, 1, 1), 'STREAM_PM_INC', 9),             # FOA, four groups
    ((1, 2048, 14, 14, 256, 256, 9, 1, 1), 'STREAM_PM_INC', 31),          # mask head
    ((1, 8, 256, 256, 256, 256, 9, 1, 1), 'STREAM_SAME', 28),
    ((1, 8192, 1, 1, 12544, 1024, 1, 1, 1), 'STREAM_DENSE', 1),           # FC 12544 -> 1024
    ((1, 8, 64, 64, 256, 256, 9, 1, 1), 'RING_SAME', 8),
    ((1, 2048, 14, 14, 256, 256, 4, 1, 2), 'STREAM_GENERIC', 64),         # mask head deconvolution
    ((1, 8, 64, 64, 256, 1024, 1, 1, 1), 'RING_DENSE', 18),
    ((1, 8, 128, 128, 128, 512, 1, 1, 1), 'RING_DENSE', 71),
    ((1, 8, 64, 64, 1024, 256, 1, 1, 1), 'RING_DENSE', 18),
    ((1, 8, 128, 128, 128, 128, 9, 1, 1), 'RING_SAME', 32),
    ((1, 8, 128, 128, 512, 128, 1, 1, 1), 'RING_DENSE', 71),
    ((1, 8, 128, 128, 512, 256, 1, 1, 1), 'RING_DENSE', 36),
    ((1, 8, 32, 32, 512, 512, 9, 1, 1), 'RING_SAME', 2),
    ((1, 8, 128, 128, 256, 256, 9, 1, 1), 'STREAM_SAME', 28),
    ((1, 8, 256, 256, 256, 256, 1, 1, 1), 'STREAM_DENSE', 256),
    ((1, 8, 256, 256, 256, 128, 1, 1, 1), 'RING_DENSE', 144),
    ((1, 8, 32, 32, 512, 2048, 1, 1, 1), 'RING_DENSE', 4),
    ((1, 8192, 1, 1, 1024, 1024, 1, 1, 1), 'RING_DENSE', 4),
    ((1, 8, 32, 32, 512, 512, 9, 2, 1), 'RING_GENERIC', 3),
    ((1, 8, 32, 32, 2048, 512, 1, 1, 1), 'RING_DENSE', 4),
    ((1, 8, 128, 128, 128, 128, 9, 2, 1), 'RING_GENERIC', 56),
    ((1, 8, 64, 64, 256, 256, 9, 2, 1), 'RING_GENERIC', 14),
    ((1, 8, 128, 128, 256, 512, 1, 2, 1), 'RING_GENERIC', 64),
    ((1, 8, 32, 32, 1024, 2048, 1, 2, 1), 'RING_GENERIC', 4),
    ((1, 8, 64, 64, 1024, 512, 1, 1, 1), 'RING_DENSE', 9),
    ((1, 8, 64, 64, 512, 1024, 1, 2, 1), 'RING_GENERIC', 16),
]


def bench_geometry(shape):
    G, B, OH, OW, Cin, Cout, T, ss, gos = shape
    if T == 4:
        taps = [(py, px, 0, 0, py * 2 + px) for py in range(2) for px in range(2)]
    else:
        R = {9: 3, 1: 1}[T]
        taps = [(0, 0, r - R // 2, s - R // 2, r * R + s) for r in range(R) for s in range(R)]
    return dict(B=B, GH=OH * gos, GW=OW * gos, Cout=Cout, XH=OH * ss, XW=OW * ss, Cin=Cin, OH=OH, OW=OW, taps=taps, gos=gos, ss=ss,
                groups=G, splits=0, variant=K.WGRAD_AUTO)


@pytest.mark.parametrize('row', BENCH, ids=['x'.join(map(str, r[0])) for r in BENCH])
def test_bench_shape_keeps_its_plan(row):
    shape, form, parent_slots = row
    geo = bench_geometry(shape)
    p = K.conv_wgrad_plan(**geo)
    assert form_name(p.form) == form, (shape, form_name(p.form))
    want = restate(**geo)
    assert want['nslots'] == parent_slots and as_dict(p) == want and slots_query(geo) == parent_slots
    assert p.grid[0] * p.grid[1] * p.grid[2] <= 512           # the split targets: 256 / 288 / 512 workgroups


def test_bench_table_has_the_headline_shapes():
    shapes = [r[0] for r in BENCH]
    for s in ((4, 2048, 7, 7, 256, 256, 9, 1, 1), (1, 2048, 14, 14, 256, 256, 9, 1, 1), (1, 2048, 14, 14, 256, 256, 4, 1, 2),
              (1, 8192, 1, 1, 12544, 1024, 1, 1, 1)):
        assert s in shapes
    assert sum(1 for s in shapes if s[1] == 8 and s[6] == 1) >= 6 and sum(1 for s in shapes if s[1] == 8 and s[6] == 9) >= 5
    assert {r[1] for r in BENCH} >= {'STREAM_PM_INC', 'STREAM_GENERIC', 'STREAM_DENSE', 'STREAM_SAME', 'RING_DENSE', 'RING_SAME', 'RING_GENERIC'}


# ------------------------------------------------------------------ operand planes

# one 128-channel and one 256-channel shape: a dense 3 x 3 layer (ring) and an RoI map in four groups (valid rows)
PLANE_SHAPES = [(1, 8, 64, 64, 128, 128, 9, 1, 1), (4, 256, 7, 7, 256, 256, 9, 1, 1)]


@pytest.mark.parametrize('shape', PLANE_SHAPES, ids=['c128_dense', 'c256_roi_groups4'])
def test_plane_launches_run_over_virtual_groups(shape):
    geo = bench_geometry(shape)
    G, T = shape[0], shape[6]
    plain = K.conv_wgrad_plan(**geo)
    last = plain.splits
    for n in (3, 6):
        p = K.conv_wgrad_plan(**geo, nterms=n)
        assert as_dict(p) == restate(**geo, nterms=n), n
        assert p.pm == plain.pm and p.grid[1] == (G * n if p.pm else T * G * n)
        # the workgroup target (same-size maps: 288, 256-tiles: 256) is divided by the VIRTUAL group count: the terms shrink the splits
        assert p.splits == max(1, (256 if p.tile == 256 else 288) // (p.grid[0] * T * G * n)) <= last
        last = p.splits
        assert p.grid[0] * p.grid[1] * p.grid[2] <= 512
    assert last < plain.splits
    # the work threshold counts them too: 256 RoIs x 49 pixels x 9 taps x 4 groups is below it, x 3 terms above
    if shape[4] == 256:
        assert form_name(plain.form) == 'T128_PM' and form_name(K.conv_wgrad_plan(**geo, nterms=3).form).startswith('STREAM_PM')


def test_plane_launches_are_refused_as_the_header_says():
    """groups * nterms <= 32, nterms <= 8, wide channels, no variant and no splits of their own."""
    geo = bench_geometry(PLANE_SHAPES[1])
    assert not refused(K.conv_wgrad_plan, **geo, nterms=8)                    # 4 x 8 = 32 virtual groups
    assert refused(K.conv_wgrad_plan, **dict(geo, groups=6), nterms=6) and refused(K.conv_wgrad_plan, **dict(geo, groups=8), nterms=6)
    assert refused(K.conv_wgrad_plan, **dict(geo, groups=1), nterms=9) and refused(K.conv_wgrad_plan, **geo, nterms=-1)
    assert refused(K.conv_wgrad_plan, **dict(geo, Cin=64), nterms=3) and refused(K.conv_wgrad_plan, **dict(geo, Cout=192), nterms=3)
    assert refused(K.conv_wgrad_plan, **dict(geo, variant=K.WGRAD_T128), nterms=3) and refused(K.conv_wgrad_plan, **dict(geo, splits=2), nterms=3)


# ------------------------------------------------------------------ both builds

def test_both_builds_make_the_same_plan():
    """The bfloat16 and the binary16 build compile the same wgrad_plan."""
    geos = [g for _, g in ROWS] + [bench_geometry(r[0]) for r in BENCH]
    bf16 = [K.conv_wgrad_plan(**g) for g in geos] + [K.conv_wgrad_plan(**bench_geometry(s), nterms=3) for s in PLANE_SHAPES]
    prev = L.set_act16(torch.float16)
    try:
        f16 = [K.conv_wgrad_plan(**g) for g in geos] + [K.conv_wgrad_plan(**bench_geometry(s), nterms=3) for s in PLANE_SHAPES]
        slots = [slots_query(g) for g in geos]
    finally:
        L.set_act16(prev)
    assert f16 == bf16 and slots == [p.nslots for p in bf16[:len(geos)]]
