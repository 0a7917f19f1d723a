"""GPU: every kernel of the forward / data-gradient tap convolution (loft_conv_tap_bf16_v: the 19 LOFT_CONV_* codes, their
LOFT_CONV_FLAG_* order / layout flags, the process-wide stream forms, and whatever LOFT_CONV_AUTO picks) against the defining sum
of include/loft_hip.h in float64, at the small ragged geometries of tests/test_conv_forms_cpu.py.  Nothing is skipped: a kernel
that does not serve a launch (serves() of that file) must refuse it -- LoftHipError, the output untouched bit for bit.  (That the
library's conv_refusal / conv_tap_plan agree with serves(), and which kernel LOFT_CONV_AUTO takes for a shape, is checked without
a GPU by tests/test_conv_tap_form_cpu.py.)

The output is the middle of a larger allocation (one image in front, one behind) pre-filled with a pattern: after every launch the
two guard images are the pattern still, and the positions outside the launch's parity class hold what they held.

  (a) integers: x, residual in [-4, 4], w in {-2, -1, 1, 2}, bias in [-8, 8], prior in [-8, 8], so that
      T * Cin * 4 * 2 + 8 + 4 + 8 < 60000: every partial sum is an exact fp32 integer in ANY order and fits both 16-bit types'
      range -- the result does not depend on K order, tile shape or split, it is the exact integer (fp32 outputs) or its one
      round-to-nearest-even (16-bit outputs).  torch.equal over the full tensor, no tolerance.
  (b) random operands rounded to the 16-bit type: per entry |got - ref| <= b (fp32 outputs), <= b + eps16 / 2 * (|ref| + b)
      (16-bit outputs), b = 2 (n + 3) 2^-24 mag + 1e-30: n in-map products (exact in fp32) added in fp32, + 3 for bias,
      residual and prior, mag the sum over absolute values, the factor 2 because the matrix core's multi-term adds need not round
      to nearest at every step (the bound of tests/test_wgrad_forms_gpu.py); then ONE rounding to the 16-bit type.  (a) cannot
      see a 16-bit intermediate between K-tiles or a product dropped and compensated; this can.
"""
import collections
import functools

import pytest
import torch

from test_conv_forms_cpu import (EPI, GEO, GEOMETRIES, KERNELS, cases_of, epilogues_of, serves, tap_reference, variant_code)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # unit roundoff of an fp32 addition
PARAMS = [(g.id, e.id, c) for g in GEOMETRIES for e in epilogues_of(g) for c in cases_of(g, e)]
IDS = [f'{g}-{e}-{c.id}' for g, e, c in PARAMS]
RAN = collections.defaultdict(set)          # kernel -> the geometries it launched on (and passed), for the count at the end


def _pattern(numel, mode, dtype):
    """What the output and its guards hold before a launch: small integers (a), multiples of 1/4 (b) -- exact in every type."""
    i = torch.arange(numel, dtype=torch.float32)
    return (((i % 17) - 8) if mode == 'int' else ((i % 251) - 125) / 4).to(dtype)


@functools.lru_cache(maxsize=None)
def _operands(gid, mode, dtype):
    """The operands of a geometry, made once and shared by every epilogue and kernel: CPU tensors in the types the launch takes."""
    geo = GEO[gid]
    gen = torch.Generator().manual_seed(7 + 31 * [g.id for g in GEOMETRIES].index(gid) + (mode == 'int'))
    xs, ws = (geo.G, geo.B, geo.IH, geo.IW, geo.Cin), (geo.G, geo.n_wtaps, geo.Cout, geo.Cin)
    os_ = (geo.G, geo.B, geo.OHf, geo.OWf, geo.Cout)
    T = max(len(la.taps) for la in geo.launches)
    if mode == 'int':
        assert T * geo.Cin * 4 * 2 + 8 + 4 + 8 < 60000
        x = torch.randint(-4, 5, xs, generator=gen).to(dtype)
        w = (torch.randint(1, 3, ws, generator=gen) * (2 * torch.randint(0, 2, ws, generator=gen) - 1)).to(dtype)     # dense: no zero weight
        bias = torch.randint(-8, 9, (geo.G, geo.Cout), generator=gen).float()
        res = torch.randint(-4, 5, os_, generator=gen).to(dtype)
        mask = torch.randint(-2, 3, os_, generator=gen).to(dtype)
    else:
        x = torch.randn(xs, generator=gen).to(dtype)
        w = (torch.randn(ws, generator=gen) * (T * geo.Cin) ** -0.5).to(dtype)
        bias = torch.randn(geo.G, geo.Cout, generator=gen)
        res = torch.randn(os_, generator=gen).to(dtype)
        mask = torch.randn(os_, generator=gen).to(dtype)
        mask[torch.rand(os_, generator=gen) < 0.1] = 0                      # <= 0 is "off": zeros as well as negatives
    return dict(x=x, w=w, bias=bias, res=res, mask=mask)


@functools.lru_cache(maxsize=None)
def _device_operands(gid, mode, dtype):
    return {k: v.cuda() for k, v in _operands(gid, mode, dtype).items()}


@functools.lru_cache(maxsize=None)
def _problem(gid, eid, mode, dtype):
    """The float64 reference of (geometry, epilogue) on the CPU, once, and what the checks need of it on the device."""
    geo, epi = GEO[gid], EPI[eid]
    O = _operands(gid, mode, dtype)
    odt = torch.float32 if epi.f32 else dtype
    img = geo.OHf * geo.OWf * geo.Cout
    pattern = _pattern((geo.G * geo.B + 2) * img, mode, odt)
    prior = pattern[img:-img].view(geo.G, geo.B, geo.OHf, geo.OWf, geo.Cout)
    ref, mag, n, own = tap_reference(O['x'], O['w'], O['bias'] if epi.bias else None, O['res'] if epi.residual else None,
                                     O['mask'] if epi.mask else None, geo, prior, relu=epi.relu, accumulate=epi.accumulate)
    P = dict(pattern=pattern.cuda(), odt=odt, own=[(own == i).cuda() for i in range(len(geo.launches))])
    if mode == 'int':
        assert ref.abs().max().item() < 60000 and torch.equal(ref, ref.round())
        P['want'] = ref.to(odt).cuda()                         # (an integer < 2^24: exact in fp32, so the one rounding to 16 bits)
    else:
        b = 2 * (n.view(geo.OHf, geo.OWf, 1) + 3) * U * mag + 1e-30
        P['ref'] = ref.cuda()
        P['bound'] = (b if epi.f32 else b + torch.finfo(dtype).eps / 2 * (ref.abs() + b)).cuda()
        P['scale'] = ref.abs().max().item()
        if epi.mask:
            off = (O['mask'].double() <= 0) & (own >= 0).view(1, 1, geo.OHf, geo.OWf, 1)
            assert off.any() and (ref[off] == 0).all()
            P['off'] = off.cuda()
    return P


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _launch(K, geo, epi, D, la, out):
    K.conv_tap(D['x'], D['w'], out, geo.B, geo.IH, geo.IW, geo.Cin, geo.Cout, la.OH, la.OW, geo.OHf, geo.OWf, list(la.taps), ss=la.ss,
               os=la.os, oo=(la.oo_y, la.oo_x), bias=D['bias'] if epi.bias else None, residual=D['res'] if epi.residual else None,
               relu=epi.relu, accumulate=epi.accumulate, groups=geo.G, src_gs=geo.B * geo.IH * geo.IW * geo.Cin,
               wgt_gs=geo.n_wtaps * geo.Cout * geo.Cin, out_gs=geo.B * geo.OHf * geo.OWf * geo.Cout, bias_gs=geo.Cout,
               mask=D['mask'] if epi.mask else None)


def _run(gid, eid, case, mode):
    """All launches of the geometry under `case` -> the output [G, B, OHf, OWf, Cout], or None when every launch was refused as
    serves() says it must be.  Guards and foreign positions are checked after every launch."""
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    geo, epi = GEO[gid], EPI[eid]
    P, D = _problem(gid, eid, mode, L.act16()), _device_operands(gid, mode, L.act16())
    img = geo.OHf * geo.OWf * geo.Cout
    buf = P['pattern'].clone()
    out = buf[img:-img].view(geo.G, geo.B, geo.OHf, geo.OWf, geo.Cout)
    ok = serves(case.kernel, case.flags, geo, epi)
    prev_variant, K.CONV_VARIANT = K.CONV_VARIANT, variant_code(case)
    prev_form = L.load().loft_conv_stream_form(case.form) if case.form is not None else None
    try:
        for li, la in enumerate(geo.launches):
            if not ok:
                with pytest.raises(L.LoftHipError):
                    _launch(K, geo, epi, D, la, out)
                torch.cuda.synchronize()
                assert torch.equal(_bits(buf), _bits(P['pattern'])), (gid, eid, case.id, li, 'a refused launch wrote')
                continue
            before = out.clone()
            _launch(K, geo, epi, D, la, out)
            assert torch.equal(_bits(buf[:img]), _bits(P['pattern'][:img])), (gid, eid, case.id, li, 'wrote in front of the output')
            assert torch.equal(_bits(buf[-img:]), _bits(P['pattern'][-img:])), (gid, eid, case.id, li, 'wrote behind the output')
            foreign = ~P['own'][li]
            assert torch.equal(_bits(out[:, :, foreign]), _bits(before[:, :, foreign])), (gid, eid, case.id, li, 'wrote outside its parity class')
    finally:
        K.CONV_VARIANT = prev_variant
        if prev_form is not None:
            L.load().loft_conv_stream_form(prev_form)
    return (out, P) if ok else (None, P)


@pytest.mark.parametrize('gid,eid,case', PARAMS, ids=IDS)
def test_exact_on_integers(gid, eid, case):
    got, P = _run(gid, eid, case, 'int')
    if got is None:
        return
    assert got.dtype == P['odt']
    if not torch.equal(got, P['want']):
        bad = (got != P['want']).nonzero()
        raise AssertionError((gid, eid, case.id, f'{len(bad)} of {got.numel()} entries differ', bad[:4].tolist(),
                              got[tuple(bad[0])].item(), P['want'][tuple(bad[0])].item()))
    RAN[case.kernel].add(gid)


@pytest.mark.parametrize('gid,eid,case', PARAMS, ids=IDS)
def test_random_against_fp64(gid, eid, case):
    got, P = _run(gid, eid, case, 'rand')
    if got is None:
        return
    err = (got.double() - P['ref']).abs()
    ratio = (err / P['bound']).max().item()
    print(f'CONV_FORM_RATIO {gid}/{eid} {case.id} {ratio:.4f} max_err={err.max().item():.3e} max_ref={P["scale"]:.3e}')
    assert ratio <= 1.0, (gid, eid, case.id, ratio)                # (NaN fails too)
    if 'off' in P:
        assert (got[P['off']] == 0).all(), (gid, eid, case.id, 'not zero where relu_mask <= 0')


def test_every_kernel_ran_on_four_geometries():
    """The count of what actually LAUNCHED (refusals do not count): each of the 19 codes and LOFT_CONV_AUTO on at least four
    geometries.  What test_exact_on_integers has not run in this process (a selected subset) runs here."""
    for k in KERNELS:
        for g in GEOMETRIES:
            if g.id in RAN[k]:
                continue
            for e in epilogues_of(g):
                if serves(k, (), g, e):
                    test_exact_on_integers(g.id, e.id, [c for c in cases_of(g, e) if c.id == k][0])
                    break
    counts = {k: len(RAN[k]) for k in KERNELS}
    print('CONV_FORM_COUNT', counts)
    assert all(c >= 4 for c in counts.values()), counts
