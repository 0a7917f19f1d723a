"""CPU: the table tests/test_conv_forms_gpu.py is parametrised over -- small ragged geometries of the forward / data-gradient
tap convolution (loft_conv_tap_bf16_v), the 19 kernel codes with their order / layout flags and stream forms, the rule that says
which kernel serves which launch (serves: the constraints include/loft_hip.h documents and conv_refusal of csrc/conv_mfma.hip
enforces; tests/test_conv_tap_form_cpu.py compares the two through loft_conv_tap_form, without a GPU) -- and the reference: the
defining sum of include/loft_hip.h written out in float64, checked here against F.conv2d, the autograd input gradient and
F.conv_transpose2d."""
import collections

import pytest
import torch
import torch.nn.functional as F

from bonai_amd import kernels as K

# One launch of loft_conv_tap_bf16: the launch iterates oy < OH, ox < OW, reads src[oy * ss + dy, ox * ss + dx] per tap
# (dy, dx, weight tap) and writes out[oy * os + oo_y, ox * os + oo_x] of the [OHf, OWf] map.
Launch = collections.namedtuple('Launch', 'OH OW ss os oo_y oo_x taps')
# groups x [B, IH, IW, Cin] -> groups x [B, OHf, OWf, Cout] with n_wtaps packed weight taps [n_wtaps][Cout][Cin]; conv = what the
# launches compute, for the self-check of the reference: ('fwd', R, stride, pad) | ('dgrad', R, stride, pad) | ('deconv',) | ('taps',)
Geo = collections.namedtuple('Geo', 'id G B Cin Cout IH IW OHf OWf n_wtaps launches conv')


def fwd_geo(gid, G, B, Cin, Cout, IH, IW, R, stride, pad):
    """K.conv2d_fwd's launch."""
    OH, OW = K.conv_out_size(IH, R, stride, pad), K.conv_out_size(IW, R, stride, pad)
    taps = tuple((r - pad, s - pad, r * R + s) for r in range(R) for s in range(R))
    return Geo(gid, G, B, Cin, Cout, IH, IW, OH, OW, R * R, (Launch(OH, OW, stride, 1, 0, 0, taps),), ('fwd', R, stride, pad))


def dgrad_geo(gid, G, B, conv_cin, conv_cout, in_h, in_w, R, stride, pad):
    """K.conv2d_dgrad's launches for a conv conv_cin -> conv_cout on an in_h x in_w input: the contraction runs over the conv's
    OUTPUT channels (Cin of the launch) and writes its input gradient; one launch per output parity class when strided."""
    GH, GW = K.conv_out_size(in_h, R, stride, pad), K.conv_out_size(in_w, R, stride, pad)
    if stride == 1:
        taps = tuple((pad - r, pad - s, r * R + s) for r in range(R) for s in range(R))
        launches = (Launch(in_h, in_w, 1, 1, 0, 0, taps),)
    else:
        launches = []
        for py in range(stride):
            for px in range(stride):
                taps = tuple(((py + pad - r) // stride, (px + pad - s) // stride, r * R + s) for r in range(R) for s in range(R)
                             if (py + pad - r) % stride == 0 and (px + pad - s) % stride == 0)
                nh, nw = (in_h - py + stride - 1) // stride, (in_w - px + stride - 1) // stride
                if taps and nh > 0 and nw > 0:
                    launches.append(Launch(nh, nw, 1, stride, py, px, taps))
        launches = tuple(launches)
    return Geo(gid, G, B, conv_cout, conv_cin, GH, GW, in_h, in_w, R * R, launches, ('dgrad', R, stride, pad))


def deconv_geo(gid, B, Cin, Cout, H, W):
    """The four parity launches of the 2x2 / stride-2 transposed convolution (nn.deconv2x2_relu): tap 2 py + px -> out[2y + py, 2x + px]."""
    launches = tuple(Launch(H, W, 1, 2, py, px, ((0, 0, py * 2 + px),)) for py in range(2) for px in range(2))
    return Geo(gid, 1, B, Cin, Cout, H, W, 2 * H, 2 * W, 4, launches, ('deconv',))


def taps_geo(gid, B, Cin, Cout, H, W, taps):
    return Geo(gid, 1, B, Cin, Cout, H, W, H, W, max(t[2] for t in taps) + 1, (Launch(H, W, 1, 1, 0, 0, tuple(taps)),), ('taps',))


# 16 taps = CONV_MAX_TAPS, weight taps 0..15 (permuted), offsets outside the packed tap table's -8..7 (pk_ok = 0): a 3x3 at
# dilation 9 plus seven more, one of which reaches only a corner of the 24 x 24 map
_FAR = [(9 * i, 9 * j) for i in (-1, 0, 1) for j in (-1, 0, 1)] + [(-1, 0), (0, 1), (5, -7), (-12, 3), (3, -12), (11, 11), (-23, 23)]
FAR_TAPS = [(dy, dx, (5 * t + 3) % 16) for t, (dy, dx) in enumerate(_FAR)]

GEOMETRIES = [
    fwd_geo('fwd3x3_ragged', 1, 2, 64, 256, 17, 19, 3, 1, 1),        # M = 646: 256 / 128 / 64 tiles + a partial one, 9 K-tiles, border taps
    fwd_geo('pw_tiny', 1, 1, 64, 256, 9, 9, 1, 1, 0),                # M = 81 < the 128- / 256-pixel tiles, ONE K-tile, the pointwise shortcut
    fwd_geo('pw_m49', 1, 1, 64, 256, 7, 7, 1, 1, 0),                 # M = 49: less than the 64-pixel tiles too
    fwd_geo('pw_s2', 1, 2, 128, 256, 15, 15, 1, 2, 0),               # 1x1 with ss = 2: its non-pointwise twin
    fwd_geo('fwd3x3_s2_n128', 1, 2, 128, 128, 16, 18, 3, 2, 1),      # Cout = 128: the stream kernel's 128-cout tiles, T128 forms
    dgrad_geo('dgrad3x3_s2', 1, 2, 256, 256, 15, 17, 3, 2, 1),       # four parity launches os = 2, 1 / 2 / 2 / 4 taps, unequal nh, nw
    deconv_geo('deconv2x2_parity', 3, 64, 256, 7, 7),                # T = 1, os = 2, four launches
    fwd_geo('roi_pixmajor', 1, 300, 64, 256, 7, 7, 3, 1, 1),         # pixel-major rows, one RoI block, taps skipped per tile
    fwd_geo('roi_two_blocks', 1, 520, 128, 256, 3, 3, 3, 1, 1),      # two RoI blocks of pm_S = 260 rows per position
    fwd_geo('roi_two_blocks_padded', 1, 521, 128, 256, 3, 3, 3, 1, 1),   # pm_S = 261: padded rows, nb * P * S > P * B
    fwd_geo('groups4', 4, 3, 64, 256, 7, 7, 3, 1, 1),                # group strides of src / wgt / out / bias
    fwd_geo('narrow16', 1, 1, 256, 16, 12, 12, 1, 1, 0),             # Cout % 4: the 128 x 64 tile only
    fwd_geo('narrow36', 1, 6, 64, 36, 9, 9, 3, 2, 1),
    taps_geo('taps16_far', 1, 64, 256, 24, 24, FAR_TAPS),
    fwd_geo('deepk', 1, 1, 512, 256, 10, 10, 3, 1, 1),               # 72 K-tiles: the FAST forms' hoisted addressing
    # 64 -> 64 channels, stride 1, taps within -1..1: what the halo patch kernel (LOFT_CONV_PATCH64) serves -- more than one
    # 16 x 16 patch with partial ones, a map smaller than a patch, four taps (its minimum), a data gradient's mirrored taps
    fwd_geo('p64_3x3_ragged', 1, 2, 64, 64, 17, 19, 3, 1, 1),
    fwd_geo('p64_tiny', 1, 1, 64, 64, 5, 5, 3, 1, 1),
    taps_geo('p64_2x2', 1, 64, 64, 16, 33, [(0, 0, 2), (0, 1, 0), (1, 0, 3), (1, 1, 1)]),
    dgrad_geo('p64_dgrad', 1, 3, 64, 64, 20, 16, 3, 1, 1),
]
GEO = {g.id: g for g in GEOMETRIES}
NARROW = ('narrow16', 'narrow36')
ROI_GEOS = ('roi_pixmajor', 'roi_two_blocks', 'roi_two_blocks_padded')

Epilogue = collections.namedtuple('Epilogue', 'id bias residual relu mask f32 accumulate')
EPILOGUES = [
    Epilogue('plain', False, False, False, False, False, False),
    Epilogue('bias_relu', True, False, True, False, False, False),
    Epilogue('bias_res_relu', True, True, True, False, False, False),
    Epilogue('res_mask', False, True, False, True, False, False),          # the data-gradient form
    Epilogue('f32', True, False, False, False, True, False),
    Epilogue('f32_acc', True, False, False, False, True, True),
]
EPI = {e.id: e for e in EPILOGUES}
ALL_EPILOGUE_GEOS = ('fwd3x3_ragged', 'dgrad3x3_s2', 'p64_3x3_ragged')     # every epilogue; the others: bias + ReLU and the plain form


def epilogues_of(geo):
    return EPILOGUES if geo.id in ALL_EPILOGUE_GEOS else [EPI['bias_relu'], EPI['plain']]


KERNELS = ['AUTO', 'PIPE256', 'T256_FAST', 'T256', 'T128_SINGLE', 'T128_FAST', 'T128', 'T128x64', 'PATCH64', 'STREAM256', 'STREAM128',
           'STREAM64', 'STREAM64N', 'ROLES256', 'STREAM256N', 'RING32', 'W4', 'XFIRST', 'LEAN', 'LEANX']
PIPELINED = ['PIPE256', 'STREAM256', 'STREAM128', 'STREAM64', 'STREAM64N', 'ROLES256', 'STREAM256N', 'RING32', 'W4', 'XFIRST', 'LEAN',
             'LEANX']
LOCKSTEP = ['T256_FAST', 'T256', 'T128_SINGLE', 'T128_FAST', 'T128', 'T128x64']

# (id, kernel, flag names, stream form | None, the geometries it runs on | None = all)
Case = collections.namedtuple('Case', 'id kernel flags form geos')
FLAG_CASES = (
    [Case(f'{k}+TAP_MAJOR', k, ('TAP_MAJOR',), None, None) for k in PIPELINED]
    + [Case(f'{k}+KROT', k, ('KROT',), None, None) for k in PIPELINED]
    + [Case(f'{k}+NO_PIXMAJOR', k, ('NO_PIXMAJOR',), None, ROI_GEOS) for k in PIPELINED + ['T256_FAST']]
    + [Case(f'{k}+NO_ROI_BLOCKS', k, ('NO_ROI_BLOCKS',), None, ROI_GEOS) for k in PIPELINED]
    + [Case(f'{k}+NO_STAGED_OUT', k, ('NO_STAGED_OUT',), None, None) for k in LOCKSTEP]
    + [Case(f'{k}+NO_NFAST', k, ('NO_NFAST',), None, None) for k in LOCKSTEP]
    # the pinned two-stage 256 x 256 stream schedule under every process-wide form (loft_conv_stream_form), 4 + 2: LEAN with the
    # plane launches' direct fp32 epilogue bit set
    + [Case(f'STREAM256@form{f}', 'STREAM256', (), f, None) for f in (0, 1, 2, 3, 6)]
    + [Case(f'STREAM256+TAP_MAJOR@form{f}', 'STREAM256', ('TAP_MAJOR',), f, ('fwd3x3_ragged', 'dgrad3x3_s2', 'roi_two_blocks_padded'))
       for f in (0, 1, 2, 3)]
)
KERNEL_CASES = [Case(k, k, (), None, None) for k in KERNELS]


def variant_code(case):
    code = getattr(K, 'CONV_' + case.kernel)
    for f in case.flags:
        code |= getattr(K, 'CONV_FLAG_' + f)
    return code


def cases_of(geo, epi):
    """The kernel / flag cases a (geometry, epilogue) runs under: every kernel code everywhere; the flag and stream-form cases on
    the bias + ReLU epilogue of their geometries."""
    out = list(KERNEL_CASES)
    if epi.id == 'bias_relu':
        out += [c for c in FLAG_CASES if c.geos is None or geo.id in c.geos]
    return out


def serves(kernel, flags, geo, epi):
    """Whether loft_conv_tap_bf16_v launches `kernel` (a KERNELS name) with `flags` (CONV_FLAG_* names) on every launch of `geo`
    with epilogue `epi`, or returns hipErrorInvalidValue -- from the constraints of include/loft_hip.h and conv_refusal
    (csrc/conv_mfma.hip).  The answer is the same for all launches of a geometry (test_serves_is_one_answer_per_geometry)."""
    return all(_serves_launch(kernel, flags, geo, la, epi) for la in geo.launches)


def _serves_launch(kernel, flags, geo, la, epi):
    if kernel in ('AUTO', 'T128x64'):
        return True                                   # Cin % 64 == 0, Cout % 4 == 0, T <= 16: the contract itself
    if kernel in PIPELINED:
        if epi.f32 or epi.accumulate:                 # their epilogue collects a 16-bit tile in LDS
            return False
        if geo.Cout % 256 and not (kernel == 'STREAM256' and geo.Cout % 128 == 0):
            return False
        if 'TAP_MAJOR' in flags and kernel in ('LEAN', 'LEANX', 'RING32', 'W4'):      # chunk-major schedules only
            return False
        if 'KROT' in flags and kernel in ('RING32', 'W4'):
            return False
        return True
    if kernel in ('T256', 'T256_FAST'):
        return geo.Cout % 256 == 0
    if kernel in ('T128', 'T128_FAST'):
        return geo.Cout % 128 == 0
    if kernel == 'T128_SINGLE':                        # one LDS tile: not residual AND mask tiles of a dense 16-bit output
        dense_out = not epi.f32 and la.os == 1 and geo.OHf == la.OH and geo.OWf == la.OW
        return geo.Cout % 128 == 0 and not (epi.residual and epi.mask and dense_out)
    if kernel == 'PATCH64':                            # 64 -> 64, one group, unit strides, same-size map, 4..9 taps within -1..1
        return (geo.Cin == 64 and geo.Cout == 64 and geo.G == 1 and 4 <= len(la.taps) <= 9 and la.ss == 1 and la.os == 1
                and la.OH == geo.IH and la.OW == geo.IW and geo.OHf == la.OH and geo.OWf == la.OW and not epi.f32 and not epi.accumulate
                and all(-1 <= t[0] <= 1 and -1 <= t[1] <= 1 for t in la.taps))
    raise KeyError(kernel)


def tap_reference(x, w, bias, residual, mask, geo, prior, relu=False, accumulate=False):
    """The defining sum of include/loft_hip.h (loft_conv_tap_bf16) in float64, all launches of `geo` one after the other.
    x [G, B, IH, IW, Cin], w [G, n_wtaps, Cout, Cin], bias [G, Cout] | None, residual / mask / prior [G, B, OHf, OWf, Cout] (None but
    for prior) -> (out, mag, n, own):
      out  [G, B, OHf, OWf, Cout] float64: prior where no launch writes; elsewhere act(bias + residual + sum), zero where
           mask <= 0, plus prior with `accumulate`;
      mag  the same sum over absolute values (bias, residual and the accumulated prior included): what a rounding error is relative to;
      n    [OHf, OWf] the number of in-map products of an output at that position;
      own  [OHf, OWf] the index of the launch that writes the position, -1: none."""
    G, B, IH, IW, Cin = x.shape
    xd, wd = x.double(), w.double()
    out = prior.double().clone()
    mag = torch.zeros_like(out)
    n = torch.zeros(geo.OHf, geo.OWf, dtype=torch.float64)
    own = torch.full((geo.OHf, geo.OWf), -1, dtype=torch.long)
    for li, la in enumerate(geo.launches):
        acc = torch.zeros(G, B, la.OH, la.OW, geo.Cout, dtype=torch.float64)
        am = torch.zeros_like(acc)
        cnt = torch.zeros(la.OH, la.OW, dtype=torch.float64)
        for dy, dx, wt in la.taps:
            ys = [oy for oy in range(la.OH) if 0 <= oy * la.ss + dy < IH]       # the output rows / columns whose source pixel is in the map
            xs = [ox for ox in range(la.OW) if 0 <= ox * la.ss + dx < IW]
            if not ys or not xs:
                continue
            y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
            sl = xd[:, :, y0 * la.ss + dy:(y1 - 1) * la.ss + dy + 1:la.ss, x0 * la.ss + dx:(x1 - 1) * la.ss + dx + 1:la.ss]
            rows = sl.reshape(G, -1, Cin)
            wn = wd[:, wt].transpose(1, 2)                                     # [G, Cin, Cout]
            acc[:, :, y0:y1, x0:x1] += (rows @ wn).view(G, B, y1 - y0, x1 - x0, geo.Cout)
            am[:, :, y0:y1, x0:x1] += (rows.abs() @ wn.abs()).view(G, B, y1 - y0, x1 - x0, geo.Cout)
            cnt[y0:y1, x0:x1] += Cin
        sy = slice(la.oo_y, la.oo_y + (la.OH - 1) * la.os + 1, la.os)
        sx = slice(la.oo_x, la.oo_x + (la.OW - 1) * la.os + 1, la.os)
        assert (own[sy, sx] == -1).all(), 'two launches write the same position'
        if bias is not None:
            acc += bias.double().view(G, 1, 1, 1, -1)
            am += bias.double().abs().view(G, 1, 1, 1, -1)
        if residual is not None:
            acc += residual.double()[:, :, sy, sx]
            am += residual.double().abs()[:, :, sy, sx]
        if relu:
            acc.clamp_(min=0)
        if mask is not None:
            acc = torch.where(mask.double()[:, :, sy, sx] > 0, acc, torch.zeros_like(acc))
        if accumulate:
            acc += out[:, :, sy, sx]
            am += out[:, :, sy, sx].abs()
        out[:, :, sy, sx] = acc
        mag[:, :, sy, sx] = am
        n[sy, sx] = cnt
        own[sy, sx] = li
    return out, mag, n, own


# ------------------------------------------------------------------ the tables

def test_tables_are_what_the_gpu_file_expects():
    assert len(KERNELS) == 20 and [getattr(K, 'CONV_' + k) for k in KERNELS] == list(range(20))
    assert set(PIPELINED) | set(LOCKSTEP) | {'AUTO', 'PATCH64'} == set(KERNELS) and len(PIPELINED) + len(LOCKSTEP) + 2 == 20
    assert len({g.id for g in GEOMETRIES}) == len(GEOMETRIES)
    ids = [c.id for c in KERNEL_CASES + FLAG_CASES]
    assert len(set(ids)) == len(ids)
    for flag in ('TAP_MAJOR', 'KROT', 'NO_PIXMAJOR', 'NO_ROI_BLOCKS', 'NO_STAGED_OUT', 'NO_NFAST'):
        assert any(flag in c.flags for c in FLAG_CASES), flag
    assert {c.form for c in FLAG_CASES if c.form is not None} == {0, 1, 2, 3, 6}
    for g in GEOMETRIES:
        assert g.Cin % 64 == 0 and g.Cout % 4 == 0
        for la in g.launches:
            assert 1 <= len(la.taps) <= 16 and all(0 <= t[2] < g.n_wtaps for t in la.taps)
            # every launch stays inside the output map it is given
            assert la.oo_y + (la.OH - 1) * la.os < g.OHf and la.oo_x + (la.OW - 1) * la.os < g.OWf


def test_geometries_reach_their_hazards():
    g = GEO['fwd3x3_ragged']
    M = g.B * g.OHf * g.OWf
    assert M == 646 and M % 64 and len(g.launches[0].taps) * g.Cin // 64 == 9
    assert GEO['pw_tiny'].B * 81 < 128 and GEO['pw_m49'].B * 49 < 64 and GEO['pw_tiny'].Cin == GEO['pw_m49'].Cin == 64     # one K-tile
    d = GEO['dgrad3x3_s2']
    assert [len(la.taps) for la in d.launches] == [1, 2, 2, 4] and {(la.OH, la.OW) for la in d.launches} == {(8, 9), (8, 8), (7, 9), (7, 8)}
    assert all(la.os == 2 and (la.OH, la.OW) != (d.OHf, d.OWf) for la in d.launches)
    assert [len(la.taps) for la in GEO['deconv2x2_parity'].launches] == [1, 1, 1, 1]
    # pixel-major rows: B >= 256 on a map of <= 1024 pixels; RoI blocks: B / 256 of them, ceil(B / blocks) rows per position
    for gid, blocks, rows, padded in (('roi_pixmajor', 1, 300, False), ('roi_two_blocks', 2, 260, False), ('roi_two_blocks_padded', 2, 261, True)):
        g = GEO[gid]
        nb = max(1, g.B // 256)
        assert g.B >= 256 and g.OHf * g.OWf <= 1024 and nb == blocks and -(-g.B // nb) == rows and (nb * rows > g.B) == padded
    t = GEO['taps16_far'].launches[0].taps
    assert len(t) == 16 and sorted(x[2] for x in t) == list(range(16)) and any(abs(x[0]) > 8 or abs(x[1]) > 8 for x in t)
    assert len(GEO['deepk'].launches[0].taps) * GEO['deepk'].Cin // 64 == 72
    assert GEO['narrow16'].Cout % 64 and GEO['narrow36'].Cout % 64 and GEO['narrow36'].Cout % 8


def test_every_kernel_serves_four_geometries_and_every_geometry_a_pipelined_kernel():
    for k in KERNELS:
        served = [g.id for g in GEOMETRIES if any(serves(k, (), g, e) for e in epilogues_of(g))]
        assert len(served) >= 4, (k, served)
    for g in GEOMETRIES:
        piped = [k for k in PIPELINED if serves(k, (), g, EPI['bias_relu'])]
        if g.id in NARROW or g.Cout % 128:
            assert piped == [], (g.id, piped)              # Cout % 128: the 128 x 64 tile (and the 64 -> 64 patch kernel) only
        else:
            assert piped, g.id
    for g in (GEO[i] for i in NARROW):
        assert [k for k in KERNELS if serves(k, (), g, EPI['bias_relu'])] == ['AUTO', 'T128x64']


def test_serves_is_one_answer_per_geometry():
    for g in GEOMETRIES:
        for e in epilogues_of(g):
            for c in cases_of(g, e):
                answers = {_serves_launch(c.kernel, c.flags, g, la, e) for la in g.launches}
                assert len(answers) == 1, (g.id, e.id, c.id)


def test_the_rule_refuses_what_the_header_says_it_refuses():
    f, d = GEO['fwd3x3_ragged'], GEO['dgrad3x3_s2']
    for k in PIPELINED:
        assert serves(k, (), f, EPI['bias_relu']) and not serves(k, (), f, EPI['f32']) and not serves(k, (), f, EPI['f32_acc'])
        assert serves(k, (), GEO['fwd3x3_s2_n128'], EPI['bias_relu']) == (k == 'STREAM256')
    assert not serves('LEAN', ('TAP_MAJOR',), f, EPI['bias_relu']) and serves('XFIRST', ('TAP_MAJOR',), f, EPI['bias_relu'])
    assert not serves('T128_SINGLE', (), f, EPI['res_mask']) and serves('T128_SINGLE', (), d, EPI['res_mask'])     # (strided output: direct stores)
    assert serves('T128_SINGLE', (), f, EPI['f32_acc'])
    assert not serves('PATCH64', (), f, EPI['bias_relu']) and serves('PATCH64', (), GEO['p64_tiny'], EPI['bias_relu'])
    assert not serves('PATCH64', (), GEO['p64_3x3_ragged'], EPI['f32'])


# ------------------------------------------------------------------ the reference against torch's own operators

def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def _nhwc5(t, G):
    """[G * B, C, H, W] -> [G, B, H, W, C]"""
    return t.permute(0, 2, 3, 1).reshape(G, t.shape[0] // G, t.shape[2], t.shape[3], t.shape[1]).contiguous()


@pytest.mark.parametrize('geo', [g for g in GEOMETRIES if g.conv[0] == 'fwd'], ids=lambda g: g.id)
def test_reference_is_conv2d(geo):
    _, R, stride, pad = geo.conv
    x = _randn(geo.G * geo.B, geo.Cin, geo.IH, geo.IW, seed=1)
    w = _randn(geo.G, geo.Cout, geo.Cin, R, R, seed=2)
    bias = _randn(geo.G, geo.Cout, seed=3)
    want = torch.cat([F.conv2d(x[g * geo.B:(g + 1) * geo.B], w[g], bias[g], stride=stride, padding=pad) for g in range(geo.G)])
    wp = torch.stack([w[g].permute(2, 3, 0, 1).reshape(R * R, geo.Cout, geo.Cin) for g in range(geo.G)])      # K.pack_w_fwd's layout
    prior = torch.zeros(geo.G, geo.B, geo.OHf, geo.OWf, geo.Cout, dtype=torch.float64)
    out, mag, n, own = tap_reference(_nhwc5(x, geo.G), wp, bias, None, None, geo, prior)
    assert _rel(out, _nhwc5(want, geo.G)) <= 1e-12
    assert (own == 0).all() and (mag >= out.abs() - 1e-9).all()
    # the products of an output: the taps inside the map x Cin -- all of them in the interior, fewer on a padded border
    assert n.max().item() == R * R * geo.Cin and (n.min().item() < n.max().item()) == (pad > 0)
    # ReLU and the ReLU-backward mask, against the same operators on torch's result
    res, mask = _randn(*prior.shape, seed=4), _randn(*prior.shape, seed=5)
    out2 = tap_reference(_nhwc5(x, geo.G), wp, bias, res, mask, geo, prior, relu=True)[0]
    want2 = torch.where(mask > 0, torch.relu(_nhwc5(want, geo.G) + res), torch.zeros_like(res))
    assert _rel(out2, want2) <= 1e-12


@pytest.mark.parametrize('geo', [g for g in GEOMETRIES if g.conv[0] == 'dgrad'], ids=lambda g: g.id)
def test_reference_is_the_autograd_input_gradient(geo):
    """All parity launches of a strided data gradient combined; positions are written once, and with `accumulate` add to prior."""
    _, R, stride, pad = geo.conv
    conv_cin, conv_cout = geo.Cout, geo.Cin
    x = _randn(geo.B, conv_cin, geo.OHf, geo.OWf, seed=6).requires_grad_(True)
    w = _randn(conv_cout, conv_cin, R, R, seed=7)
    g = _randn(geo.B, conv_cout, geo.IH, geo.IW, seed=8)
    y = F.conv2d(x, w, None, stride=stride, padding=pad)
    assert tuple(y.shape[2:]) == (geo.IH, geo.IW)
    (want,) = torch.autograd.grad(y, x, g)
    wpt = w.permute(2, 3, 1, 0).reshape(1, R * R, conv_cin, conv_cout)                                    # K.pack_w_dgrad's layout
    prior = _randn(1, geo.B, geo.OHf, geo.OWf, geo.Cout, seed=9)
    out, _, _, own = tap_reference(_nhwc5(g, 1), wpt, None, None, None, geo, prior)
    assert (own >= 0).all() and len(set(own.flatten().tolist())) == len(geo.launches)
    assert _rel(out, _nhwc5(want, 1)) <= 1e-12
    acc = tap_reference(_nhwc5(g, 1), wpt, None, None, None, geo, prior, accumulate=True)[0]
    assert _rel(acc, _nhwc5(want, 1) + prior) <= 1e-12


def test_reference_is_conv_transpose2d():
    geo = GEO['deconv2x2_parity']
    x = _randn(geo.B, geo.Cin, geo.IH, geo.IW, seed=10)
    w = _randn(geo.Cin, geo.Cout, 2, 2, seed=11)
    bias = _randn(1, geo.Cout, seed=12)
    want = F.conv_transpose2d(x, w, bias[0], stride=2)
    wp = w.permute(2, 3, 1, 0).reshape(1, 4, geo.Cout, geo.Cin)                 # tap 2 py + px
    prior = _randn(1, geo.B, geo.OHf, geo.OWf, geo.Cout, seed=13)
    out, _, n, own = tap_reference(_nhwc5(x, 1), wp, bias, None, None, geo, prior)
    assert _rel(out, _nhwc5(want, 1)) <= 1e-12
    assert (n == geo.Cin).all() and own[0::2, 0::2].eq(0).all() and own[0::2, 1::2].eq(1).all() and own[1::2, 0::2].eq(2).all()


def test_reference_on_free_tap_tables_is_the_sum_written_as_loops():
    """The tap tables no torch operator has (16 far taps; four taps at 0..1): sampled outputs against the sum as python loops."""
    for geo in (GEO['taps16_far'], GEO['p64_2x2']):
        la = geo.launches[0]
        x = _randn(1, geo.B, geo.IH, geo.IW, geo.Cin, seed=14)
        w = _randn(1, geo.n_wtaps, geo.Cout, geo.Cin, seed=15)
        prior = torch.zeros(1, geo.B, geo.OHf, geo.OWf, geo.Cout, dtype=torch.float64)
        out, _, n, _ = tap_reference(x, w, None, None, None, geo, prior)
        pix = [(0, 0), (0, geo.OWf - 1), (geo.OHf - 1, 0), (geo.OHf - 1, geo.OWf - 1), (geo.OHf // 2, geo.OWf // 2), (1, 9), (13, 4), (7, geo.OWf - 2)]
        for oy, ox in pix:
            want, cnt = torch.zeros(geo.Cout, dtype=torch.float64), 0
            for dy, dx, wt in la.taps:
                iy, ix = oy + dy, ox + dx
                if 0 <= iy < geo.IH and 0 <= ix < geo.IW:
                    want += w[0, wt] @ x[0, 0, iy, ix]
                    cnt += geo.Cin
            assert _rel(out[0, 0, oy, ox], want) <= 1e-12 and n[oy, ox].item() == cnt, (geo.id, oy, ox)


def test_reference_leaves_what_a_launch_does_not_own():
    """One parity launch alone: the other three classes come back as prior, bit for bit."""
    geo = GEO['dgrad3x3_s2']
    one = geo._replace(launches=geo.launches[3:])
    g = _randn(1, geo.B, geo.IH, geo.IW, geo.Cin, seed=16)
    w = _randn(1, 9, geo.Cout, geo.Cin, seed=17)
    prior = _randn(1, geo.B, geo.OHf, geo.OWf, geo.Cout, seed=18)
    out, mag, n, own = tap_reference(g, w, None, None, None, one, prior)
    keep = own == -1
    assert keep.sum().item() == geo.OHf * geo.OWf - 7 * 8 and (own[1::2, 1::2] == 0).all()
    assert torch.equal(out[:, :, keep], prior[:, :, keep]) and (mag[:, :, keep] == 0).all() and (n[keep] == 0).all()
    assert not torch.equal(out[:, :, ~keep], prior[:, :, ~keep])
