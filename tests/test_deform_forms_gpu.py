"""GPU: every kernel form of the DCNv2 sampler (csrc/deform.hip) against the defining sums in float64, at the small ragged shapes
of tests/test_deform_forms_cpu.py (FORMS x GEOS).  Each case first asks the dispatcher (K.mdcn_bwd_form) that the forced variant
reaches the kernel the row names, then runs the forward kernel and that backward kernel

  (A) on lattice operands (offsets integers or half-integers, mask logits 0 | +20 = a mask of exactly 0.5 | 1.0, x and dcol integers
      of magnitude <= 4): every bilinear weight, product and partial sum is a small dyadic number, exact in fp32 (and in the 16-bit
      forward output) in any summation order, so col, dx, d(offset), d(mask logit) must EQUAL the reference.  No tolerance;
  (B) on random operands (rounded to the operand type first): every element within a bound counted from the roundings, below;
  (C) under LOFT_MDCN_AUTO against the form AUTO resolves to, bit for bit, where no float atomic runs (tiled forms, no sample
      leaving its tile window).

The inputs (make_om) are built, not drawn: position classes rotate over (tap, pixel in tile, group), so that every tile holds
fractional offsets under a pixel, samples inside the map 12-14 pixels from their tap (beyond the tile window + margin: the binned
kernel's far branch, the window kernel's atomic fallback), samples in the border strips (-1, 0) and (H-1, H) with two and with three
corners off the map, samples at exactly -1 and exactly H / W (the strict predicates: zero value, zero gradients), samples off the map
altogether, integer positions (zero-weight corners), and mask logits 0, +20, -20 and ordinary.  census() counts the classes from
the finished tensor and the tests assert them per tile -- per tile with at least 18 (pixel, group, tap) items, which is every tile
of the 3 x 3 geometries (the smallest, 2 x 1 pixels at stride 2, has exactly 18).  Exempt are the one-tap geometry's 8 x 1-pixel
tiles (8 items per group) and its 3 x 1-pixel corner tile (3): fewer items than classes; they are held to at least three different
position classes.  Both values of each strict predicate (-1 and H, -1 and W) are asserted per map.  A far sample needs a 19- or
17-long axis.

The reference forms the sample position as the kernels do -- ONE fp32 addition of the integer tap position and the fp32 offset,
then floor and the (exact) subtraction -- so floor and the inside test agree on both sides; everything after that is float64.

Bounds of (B), u = 2^-24, per element |got - ref| <= (n + c) u mag (first order in u, as the issue states it), mag = the same sum over
absolute values, n = the number of terms of the element's sum (n terms pass through at most n - 1 additions however they are grouped: lane
partials, wave sums, chunks, splits, slabs, tile windows, atomics), c = the roundings of one term:
  * bilinear weight w = (1 - lh)(1 - lw): 3 (two subtractions, one product; lh = h - floor(h) itself is exact);
  * sigmoid 1 / (1 + expf(-l)): expf is documented at 1 ulp (HIP math API, single precision) = 2 u; the addition 1 u; the division
    is correctly rounded by default but budgeted as approximate at 2.5 ulp = 5 u: C_SIG = 8;
  * one per product.
  col:            c = 3 + 1 (w v) + 1 (x mask) + 8 = 13,  n = corners on the map (<= 4).  The 16-bit col adds one rounding of that
                  type: u16 |ref| (u16 = half an ulp: 2^-8 bfloat16, 2^-11 binary16 + half its subnormal step, 2^-25).
  dx:             c = 3 + 1 (w mask) + 1 (x dcol) + 8 = 13,  n = contributions landing on the element.
  d(offset):      term = dcol mask ((v2 - v0)(1 - lw) + (v3 - v1) lw): the longer half 3 (difference, 1 - lw, product), + 1 (sum of
                  the halves) + 1 (x dcol) + 1 (x mask) + 8 = 14,  n = channels of the deformable group.
  d(mask logit):  mask (1 - mask) sum_c dcol val_c, val = sum of four w v: 3 + 1 + 3 (corner additions) + 1 (x dcol) = 8 per term,
                  then x mask (1 + 8), 1 - mask (1), x (1 - mask) (1): c = 19,  n = channels; plus the ABSOLUTE term
                  8 u mask^2 sum|dcol val| for the cancellation in 1 - mask (the sigmoid's error is relative to mask, not to
                  1 - mask: at logit +20 the fp32 mask is exactly 1 and the gradient exactly 0, the reference's 2e-9 x sum).
16-bit operands change nothing: products of two 16-bit values are exact in fp32 and every backward output is fp32.
"""
import functools

import pytest
import torch

from test_deform_forms_cpu import B, CASES, CASE_IDS, FAMILY, GEOS, dtype_of, expected_form, geometry, variant_of

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_SIG = 8
C_COL, C_DX, C_OFF, C_MASK = 5 + C_SIG, 5 + C_SIG, 6 + C_SIG, 11 + C_SIG
FRAC, FAR_Y, STRIP_Y, STRIP_X, STRIP_YX, EDGE, OUTSIDE, INTEGER, FAR_X = range(9)


def gamma(k):
    """(n + c) 2^-24: the linear bound, without the 1 / (1 - k u) of the standard gamma_k."""
    return k * U


def _tile_edge(geo):
    return 8 if GEOS[geo][3] == 1 else 4


def _grids(geo, DG):
    """Index grids [B, OH, OW, DG, K] (broadcastable) and the integer tap positions (ty, tx)."""
    IH, IW, k, stride, pad, dil = GEOS[geo]
    s = geometry(geo, 64, DG)
    OH, OW, KK = s['OH'], s['OW'], k * k
    b = torch.arange(B).view(B, 1, 1, 1, 1)
    oy = torch.arange(OH).view(1, OH, 1, 1, 1)
    ox = torch.arange(OW).view(1, 1, OW, 1, 1)
    g = torch.arange(DG).view(1, 1, 1, DG, 1)
    kk = torch.arange(KK).view(1, 1, 1, 1, KK)
    ty = oy * stride - pad + (kk // k) * dil
    tx = ox * stride - pad + (kk % k) * dil
    return b, oy, ox, g, kk, ty, tx


def _sample_points(om, geo, DG):
    """om fp32 [B, OH, OW, >= 3 DG K] -> the kernels' view of every (pixel, group, tap): position (one fp32 addition), inside test,
    top-left corner, fractions, the four corners' coordinates and whether they lie on the map; all [B, OH, OW, DG, K(, 4)]."""
    IH, IW, k = GEOS[geo][:3]
    KK = k * k
    Bn, OH, OW, _ = om.shape
    _, _, _, _, _, ty, tx = _grids(geo, DG)
    off = om[..., :2 * DG * KK].reshape(Bn, OH, OW, DG, KK, 2)
    ml = om[..., 2 * DG * KK:3 * DG * KK].reshape(Bn, OH, OW, DG, KK)
    h = ty.float() + off[..., 0]
    w = tx.float() + off[..., 1]
    assert h.dtype == torch.float32
    inside = (h > -1) & (w > -1) & (h < IH) & (w < IW)
    hf, wf = torch.floor(h), torch.floor(w)
    lh, lw = (h - hf).double(), (w - wf).double()
    hl, wl = hf.long(), wf.long()
    py = torch.stack([hl, hl, hl + 1, hl + 1], -1)
    px = torch.stack([wl, wl + 1, wl, wl + 1], -1)
    valid = inside.unsqueeze(-1) & (py >= 0) & (py <= IH - 1) & (px >= 0) & (px <= IW - 1)
    wts = torch.stack([(1 - lh) * (1 - lw), (1 - lh) * lw, lh * (1 - lw), lh * lw], -1)
    return dict(h=h, w=w, dy=off[..., 0], dx=off[..., 1], ml=ml, inside=inside, lh=lh, lw=lw, py=py, px=px, valid=valid, wts=wts)


def _leaves_window(S, geo):
    """Per (pixel, group, tap): a corner on the map with a non-zero weight lies outside the LDS window of the pixel's output tile
    (tile receptive field + 2-pixel margin: deform.hip's WH x WW at (wy0, wx0))."""
    IH, IW, k, stride, pad, dil = GEOS[geo]
    T = _tile_edge(geo)
    _, oy, ox, _, _, _, _ = _grids(geo, 1)
    wy0 = (oy // T * T * stride - pad - 2).unsqueeze(-1)
    wx0 = (ox // T * T * stride - pad - 2).unsqueeze(-1)
    WH = (T - 1) * stride + (k - 1) * dil + 6
    out = (S['py'] < wy0) | (S['py'] >= wy0 + WH) | (S['px'] < wx0) | (S['px'] >= wx0 + WH)
    return (out & S['valid'] & (S['wts'] != 0)).any(-1)


@functools.lru_cache(maxsize=None)
def make_om(geo, DG, lattice, far=True):
    """-> raw conv_offset output fp32 [B, OH, OW, 3 DG K] (offsets dy, dx per tap, then mask logits).  lattice: offsets on the
    half-integer lattice, logits 0 | +20.  far=False: every sample that would leave its tile window gets a fractional offset."""
    IH, IW, k, stride, pad, dil = GEOS[geo]
    KK = k * k
    b, oy, ox, g, kk, ty, tx = _grids(geo, DG)
    OH, OW = oy.shape[1], ox.shape[2]
    shape = (B, OH, OW, DG, KK)
    gen = torch.Generator().manual_seed(4000 + 97 * sorted(GEOS).index(geo) + 7 * DG + lattice)
    T = _tile_edge(geo)
    ly, lx = oy % T, ox % T
    cls = ((kk + lx + 2 * ly + 4 * g + b) % 9).expand(shape)
    mcls = ((kk + 2 * lx + ly + g) % 4).expand(shape)
    alt = ((kk + lx + ly) % 2 == 0).expand(shape)               # which of a class's two sides
    alt2 = ((kk + lx + ly) // 2 % 2 == 0).expand(shape)
    ty, tx = ty.expand(shape).double(), tx.expand(shape).double()
    if lattice:
        fy = fx = torch.full(shape, 0.5, dtype=torch.float64)
    else:
        fy = torch.rand(shape, generator=gen, dtype=torch.float64) * 0.8 + 0.1
        fx = torch.rand(shape, generator=gen, dtype=torch.float64) * 0.8 + 0.1
    sy = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    sx = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    frac_y, frac_x = sy * fy, sx * fx
    dy, dx = frac_y.clone(), frac_x.clone()

    def put(sel, ny=None, nx=None):
        if ny is not None:
            dy[sel] = ny[sel]
        if nx is not None:
            dx[sel] = nx[sel]

    want = (12 + (kk + lx) % 2).expand(shape).double()         # 12 + f or 13 + f pixels away, f in (0, 1): inside (12, 14)
    for c, t, n, d in ((FAR_Y, ty, IH, 0), (FAR_X, tx, IW, 1)):
        f = fy if d == 0 else fx
        for delta in (want, 25 - want):                         # the other distance where the first does not fit
            up, dn = t + delta + 1 <= n - 1, t - delta - 1 >= 0
            far_off = torch.where(up, delta + f, -(delta + f))
            sel = (cls == c) & (up | dn) & ((dy if d == 0 else dx).abs() < 1)
            put(sel, far_off if d == 0 else None, far_off if d == 1 else None)
    strip_y = torch.where(alt, -1 + fy, IH - 1 + fy) - ty         # h in (-1, 0) | (IH - 1, IH)
    strip_x = torch.where(alt2, IW - 1 + fx, -1 + fx) - tx
    put(cls == STRIP_Y, strip_y, None)
    put(cls == STRIP_X, None, strip_x)
    put(cls == STRIP_YX, strip_y, strip_x)
    edge_y = torch.where(alt2, torch.full_like(ty, -1.0), torch.full_like(ty, float(IH))) - ty      # exactly -1 | exactly IH
    edge_x = torch.where(alt2, torch.full_like(tx, float(IW)), torch.full_like(tx, -1.0)) - tx
    put((cls == EDGE) & alt, edge_y, None)
    put((cls == EDGE) & ~alt, None, edge_x)
    out_y = torch.where(alt2, -3 - fy, IH + 2 + fy) - ty
    out_x = torch.where(alt2, IW + 4 + fx, -2 - fx) - tx
    put((cls == OUTSIDE) & alt, out_y, None)
    put((cls == OUTSIDE) & ~alt, out_y, out_x)
    put(cls == INTEGER, torch.randint(-1, 2, shape, generator=gen).double(), torch.randint(-1, 2, shape, generator=gen).double())
    ml = torch.randn(shape, generator=gen, dtype=torch.float64)
    ml[mcls == 1] = 0.0
    ml[mcls == 2] = 20.0
    ml[mcls == 3] = -20.0
    if lattice:
        ml = torch.where(mcls >= 2, 20.0, 0.0).double().expand(shape).clone()

    def pack(dy, dx):
        off = torch.stack([dy, dx], -1).reshape(B, OH, OW, DG * KK * 2)
        return torch.cat([off, ml.reshape(B, OH, OW, DG * KK)], -1).float().contiguous()

    om = pack(dy, dx)
    if not far:
        away = _leaves_window(_sample_points(om, geo, DG), geo)
        dy[away] = frac_y[away]
        dx[away] = frac_x[away]
        om = pack(dy, dx)
        assert not _leaves_window(_sample_points(om, geo, DG), geo).any()
    return om


def census(om, geo, DG, lattice):
    """Count the classes FROM THE TENSOR and hold every tile (with >= 18 items) to at least one of each."""
    IH, IW, k = GEOS[geo][:3]
    S = _sample_points(om, geo, DG)
    T = _tile_edge(geo)
    h, w, dy, dx, inside = S['h'], S['w'], S['dy'], S['dx'], S['inside']
    off_map = 4 - S['valid'].sum(-1)
    edge = (h == -1) | (h == IH) | (w == -1) | (w == IW)
    strip = inside & ((h < 0) | (h > IH - 1) | (w < 0) | (w > IW - 1))
    whole = (dy == dy.round()) & (dx == dx.round())
    classes = {
        'fractional': (dy.abs() < 1) & (dx.abs() < 1) & ~whole,
        'strip_2_corners_off': strip & (off_map == 2),
        'strip_3_corners_off': strip & (off_map == 3),
        'exact_edge': edge & ~inside,
        'outside': ~inside & ~edge,
        'integer_position': inside & (S['lh'] == 0) & (S['lw'] == 0),
        'logit_0': S['ml'] == 0,
        'logit_+20': S['ml'] == 20,
    }
    if not lattice:
        classes['logit_-20'] = S['ml'] == -20
        classes['logit_ordinary'] = (S['ml'] != 0) & (S['ml'].abs() < 10)
    else:
        half = (2 * dy == (2 * dy).round()) & (2 * dx == (2 * dx).round())
        assert half.all() and ((S['ml'] == 0) | (S['ml'] == 20)).all()
    if IH >= 17:
        classes['far_12_to_14_along_y'] = inside & (dy.abs() >= 12) & (dy.abs() <= 14)
        classes['leaves_tile_window'] = _leaves_window(S, geo)
    _, oy, ox, _, _, _, _ = _grids(geo, DG)
    OH, OW = oy.shape[1], ox.shape[2]
    ntx = -(-OW // T)
    tile = ((oy // T) * ntx + ox // T).expand(h.shape)
    ntiles = -(-OH // T) * ntx
    items = torch.zeros(ntiles, dtype=torch.long).index_add_(0, tile[0].reshape(-1), torch.ones(tile[0].numel(), dtype=torch.long))
    counts = {}
    for name, sel in classes.items():
        per = torch.zeros(B, ntiles, dtype=torch.long)
        for bb in range(B):
            per[bb].index_add_(0, tile[bb].reshape(-1), sel[bb].reshape(-1).long())
        counts[name] = per
        assert sel.any(), (geo, name)
        assert (per[:, items >= 18] >= 1).all(), (geo, name, per.tolist())
    # each side of the strict predicates occurs (a 2 x 1-pixel tile has two edge items: per map, not per tile)
    for name, sel in (('h == -1', h == -1), ('h == IH', h == IH), ('w == -1', w == -1), ('w == IW', w == IW)):
        assert (sel & ~inside).any(), (geo, name)
    # the tiles too small for nine classes (one-tap geometry: 8 x 1 and 3 x 1 pixels) still hold three different position classes
    position = torch.stack([counts[n] for n in ('fractional', 'strip_2_corners_off', 'strip_3_corners_off', 'exact_edge', 'outside',
                                                'integer_position')] + ([counts['far_12_to_14_along_y']] if IH >= 17 else []))
    held = (position >= 1).sum(0)
    assert (held[:, items < 18] >= 3).all(), (geo, held.tolist())
    if IH >= 17:
        far_x = inside & (dx.abs() >= 12) & (dx.abs() <= 14)
        assert far_x.any(), geo
        counts['far_12_to_14_along_x'] = far_x.sum()
    return counts


@functools.lru_cache(maxsize=5)
def _problem(geo, C, DG, kind, lattice):
    """Operands (rounded to the operand type) and, in float64 on the CPU, the defining sums with their |.| sums and term counts.
    Made once per (geometry, C, groups, type) and shared by every kernel form of that shape (CASES keeps them adjacent)."""
    from bonai_amd import lib as L
    dt = dtype_of(kind)
    IH, IW, k = GEOS[geo][:3]
    KK, Cg = k * k, C // DG
    om = make_om(geo, DG, lattice)
    census(om, geo, DG, lattice)
    _, OH, OW, _ = om.shape
    gen = torch.Generator().manual_seed(5000 + C + 13 * DG + lattice + 3 * sorted(GEOS).index(geo))
    if lattice:
        x = torch.randint(-4, 5, (B, IH, IW, C), generator=gen).to(dt)
        dcol = torch.randint(-4, 5, (B, OH, OW, KK, C), generator=gen).to(dt)
    else:
        x = torch.randn(B, IH, IW, C, generator=gen).to(dt)
        dcol = torch.randn(B, OH, OW, KK, C, generator=gen).to(dt)
    S = _sample_points(om, geo, DG)
    if lattice:
        mask = torch.where(S['ml'] == 0, 0.5, 1.0).double()        # 1 / (1 + expf(-20)) = 1 / (1 + 2.06e-9) = 1.0f
    else:
        mask = torch.sigmoid(S['ml'].double())
    lh, lw = S['lh'], S['lw']
    wv = S['wts'] * S['valid']                                     # [B,OH,OW,DG,K,4]; zero weight = no term
    flat = (S['py'].clamp(0, IH - 1) * IW + S['px'].clamp(0, IW - 1)).permute(0, 3, 1, 2, 4, 5).reshape(B, DG, -1)
    xg = x.double().view(B, IH * IW, DG, Cg).permute(0, 2, 1, 3)   # [B,DG,P,Cg]
    idx = flat.unsqueeze(-1).expand(-1, -1, -1, Cg)
    v = torch.gather(xg, 2, idx).view(B, DG, OH, OW, KK, 4, Cg)
    g5 = lambda t: t.permute(0, 3, 1, 2, 4)                        # noqa: E731  [B,OH,OW,DG,K] -> [B,DG,OH,OW,K]
    wv = wv.permute(0, 3, 1, 2, 4, 5).unsqueeze(-1)                # [B,DG,OH,OW,K,4,1]
    v = v * S['valid'].permute(0, 3, 1, 2, 4, 5).unsqueeze(-1)     # a corner off the map reads as zero
    mk = g5(mask).unsqueeze(-1)                                    # [B,DG,OH,OW,K,1]
    d = dcol.double().view(B, OH, OW, KK, DG, Cg).permute(0, 4, 1, 2, 3, 5)      # [B,DG,OH,OW,K,Cg]
    val, val_abs = (wv * v).sum(-2), (wv * v.abs()).sum(-2)

    def to_col(t):                                                 # [B,DG,OH,OW,K,Cg] -> [B,OH,OW,K,C]
        return t.permute(0, 2, 3, 4, 1, 5).reshape(B, OH, OW, KK, C)

    P = dict(x=x, om=om, dcol=dcol, lattice=lattice)
    P['col'], P['col_mag'] = to_col(mk * val), to_col(mk * val_abs)
    P['col_n'] = to_col(((wv != 0).sum(-2)).expand(-1, -1, -1, -1, -1, Cg).double())
    # dx: scatter the contributions mask w dcol on the corner pixels
    dxr, dxm = torch.zeros(B, DG, IH * IW, Cg, dtype=torch.float64), torch.zeros(B, DG, IH * IW, Cg, dtype=torch.float64)
    contrib_w = (mk.unsqueeze(-2) * wv)                            # [B,DG,OH,OW,K,4,1]
    dxr.scatter_add_(2, idx, (contrib_w * d.unsqueeze(-2)).reshape(B, DG, -1, Cg))
    dxm.scatter_add_(2, idx, (contrib_w * d.abs().unsqueeze(-2)).reshape(B, DG, -1, Cg))
    dxn = torch.zeros(B, DG, IH * IW, dtype=torch.float64).scatter_add_(2, flat, (wv != 0).double().reshape(B, DG, -1))
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, IH, IW, C)   # noqa: E731
    P['dx'], P['dx_mag'] = back(dxr), back(dxm)
    P['dx_n'] = back(dxn.unsqueeze(-1).expand(-1, -1, -1, Cg))
    # offsets and mask logits
    hw_, lw_, hh_, lh_ = (g5(t).unsqueeze(-1) for t in (1 - lw, lw, 1 - lh, lh))
    v0, v1, v2, v3 = v.unbind(-2)
    a0, a1, a2, a3 = v0.abs(), v1.abs(), v2.abs(), v3.abs()
    ddy = (mk * d * ((v2 - v0) * hw_ + (v3 - v1) * lw_)).sum(-1)
    ddx = (mk * d * ((v1 - v0) * hh_ + (v3 - v2) * lh_)).sum(-1)
    ddy_m = (mk * d.abs() * ((a2 + a0) * hw_ + (a3 + a1) * lw_)).sum(-1)
    ddx_m = (mk * d.abs() * ((a1 + a0) * hh_ + (a3 + a2) * lh_)).sum(-1)
    m1 = mk.squeeze(-1)
    sdm, sdm_abs = (d * val).sum(-1), (d.abs() * val_abs).sum(-1)
    one_minus = (0.5 * (m1 == 0.5) if lattice else 1 - m1)           # lattice: 1 - 1.0f = 0, exactly as fp32 has it
    dml, dml_m = m1 * one_minus * sdm, m1 * one_minus * sdm_abs
    dml_abs = m1 * m1 * sdm_abs

    def to_om(off_y, off_x, logit):                                # [B,DG,OH,OW,K] x 3 -> [B,OH,OW,3 DG K]
        off = torch.stack([off_y, off_x], -1).permute(0, 2, 3, 1, 4, 5).reshape(B, OH, OW, 2 * DG * KK)
        return torch.cat([off, logit.permute(0, 2, 3, 1, 4).reshape(B, OH, OW, DG * KK)], -1)

    P['dom'] = to_om(ddy, ddx, dml)
    P['dom_bound'] = to_om(gamma(Cg + C_OFF) * ddy_m, gamma(Cg + C_OFF) * ddx_m, gamma(Cg + C_MASK) * dml_m + C_SIG * U * dml_abs)
    if lattice:     # the reference is representable: what the kernels must return bit for bit
        for name in ('col', 'dx', 'dom'):
            assert torch.equal(P[name].float().double(), P[name]), name
        if kind == '16':
            assert torch.equal(P['col'].to(L.act16()).double(), P['col'])
    return P


def _dev(P, s, padded):
    """The operands as the channels_last device tensors the wrappers take; om padded to s['omc'] channels (padding = 7.0: ignored)."""
    x = P['x'].permute(0, 3, 1, 2).cuda()
    Bn, OH, OW, KK, C = P['dcol'].shape
    dcol = P['dcol'].reshape(Bn, OH, OW, KK * C).permute(0, 3, 1, 2).cuda()
    om = torch.full((Bn, OH, OW, s['omc']), 7.0)
    om[..., :P['om'].shape[-1]] = P['om']
    return x, om.permute(0, 3, 1, 2).cuda(), dcol


def _run(K, P, row, geo, variant):
    s = geometry(geo, row[2], row[3], row[6])
    x, om, dcol = _dev(P, s, row[6])
    args = (s['kh'], s['kw'], s['stride'], s['pad'], s['dil'], s['deform_groups'])
    col = K.mdcn_sample_fwd(x, om, *args)
    dx, dom = K.mdcn_sample_bwd(x, om, dcol, *args, variant=variant)
    nch = P['om'].shape[-1]
    Bn, OH, OW, KK, C = P['dcol'].shape
    col = col.permute(0, 2, 3, 1).reshape(Bn, OH, OW, KK, C).cpu()
    dx, dom = dx.permute(0, 2, 3, 1).cpu(), dom.permute(0, 2, 3, 1).cpu()
    assert dx.dtype == torch.float32 and dom.dtype == torch.float32 and col.dtype == P['x'].dtype
    assert torch.equal(dom[..., nch:], torch.zeros_like(dom[..., nch:])), 'padding channels of doffmask'
    return col, dx, dom[..., :nch]


def _reaches(K, row, geo):
    s = geometry(geo, row[2], row[3], row[6])
    assert K.mdcn_bwd_form(dtype=dtype_of(row[1]), variant=variant_of(row), **s) == expected_form(row, geo), row[0]


def _where(a, b):
    return (a != b).nonzero()[:4].tolist()


@pytest.mark.parametrize('row,geo', CASES, ids=CASE_IDS)
def test_lattice_operands_are_exact(row, geo):
    from bonai_amd import kernels as K
    _reaches(K, row, geo)
    P = _problem(geo, row[2], row[3], row[1], True)
    col, dx, dom = _run(K, P, row, geo, variant_of(row))
    assert torch.equal(col.double(), P['col']), ('col', _where(col.double(), P['col']))
    assert torch.equal(dx.double(), P['dx']), ('dx', _where(dx.double(), P['dx']))
    assert torch.equal(dom.double(), P['dom']), ('doffmask', _where(dom.double(), P['dom']))


@pytest.mark.parametrize('row,geo', CASES, ids=CASE_IDS)
def test_random_operands_within_rounding(row, geo):
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    _reaches(K, row, geo)
    P = _problem(geo, row[2], row[3], row[1], False)
    col, dx, dom = _run(K, P, row, geo, variant_of(row))
    b_col = gamma(P['col_n'] + C_COL) * P['col_mag']
    if row[1] == '16':
        u16, tiny = (2.0 ** -8, 0.0) if L.act16() == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
        b_col = b_col + u16 * (P['col'].abs() + b_col) + tiny
    b_dx = gamma(P['dx_n'] + C_DX) * P['dx_mag']
    ratios = {}
    for name, got, ref, bound in (('col', col, P['col'], b_col), ('dx', dx, P['dx'], b_dx), ('doffmask', dom, P['dom'], P['dom_bound'])):
        err = (got.double() - ref).abs()
        assert torch.isfinite(got).all(), name
        ratios[name] = (err / (bound + 1e-300)).max().item()
        assert (err[bound == 0] == 0).all(), (name, 'no term, yet not zero')
    print(f'MDCN_FORM_RATIO {row[0]}-{geo} ' + ' '.join(f'{k}={v:.4f}' for k, v in ratios.items()))
    for name, r in ratios.items():
        assert r <= 1.0, (row[0], geo, name, r)


def _auto_cases():
    """One case per distinct (operand type, C, padded, geometry) of the tiled rows: AUTO's choice does not depend on the row's count."""
    seen, out = set(), []
    for row, geo in CASES:
        key = (row[1], row[2], row[6], geo)
        if row[4] != 'GENERIC' and key not in seen:
            seen.add(key)
            out.append((row, geo))
    return out


@pytest.mark.parametrize('row,geo', _auto_cases(), ids=[f'{r[4].lower()}_c{r[2]}{"_padded" if r[6] else ""}-{g}' for r, g in _auto_cases()])
def test_auto_is_the_form_it_resolves_to(row, geo):
    """LOFT_MDCN_AUTO and the forced form mdcn_bwd_form says it resolves to, bit for bit (tiled forms, no sample leaves its
    window: no float atomic runs)."""
    from bonai_amd import kernels as K
    s = geometry(geo, row[2], row[3], row[6])
    dt = dtype_of(row[1])
    fam, count, edge = K.mdcn_bwd_form(dtype=dt, **s)
    assert fam == FAMILY[row[4]] and edge == _tile_edge(geo)
    gen = torch.Generator().manual_seed(6000 + row[2])
    om = make_om(geo, row[3], False, far=False)
    IH, IW, k = GEOS[geo][:3]
    P = dict(om=om, x=torch.randn(B, IH, IW, row[2], generator=gen).to(dt),
             dcol=torch.randn(B, s['OH'], s['OW'], k * k, row[2], generator=gen).to(dt))
    _, dx0, dom0 = _run(K, P, row, geo, K.MDCN_AUTO)
    _, dx1, dom1 = _run(K, P, row, geo, K.mdcn_variant(fam, count))
    assert torch.equal(dx0, dx1) and torch.equal(dom0, dom1)
