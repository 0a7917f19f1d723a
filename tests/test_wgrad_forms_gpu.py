"""GPU: every kernel of the 16-bit weight-gradient family against the defining sum of include/loft_hip.h (loft_conv_wgrad_bf16),
at the small ragged shapes of tests/test_wgrad_forms_cpu.py.  Each case first asks the dispatcher (K.conv_wgrad_form) that its
shape still reaches the kernel it was written for, then runs that kernel

  (a) on random operands: every entry of dW and of the fused bias gradient against the same sum in float64 on the CPU, within
      the rounding of the fp32 additions alone (the products of two 16-bit values are exact in fp32); the split-K slots mode of
      the same kernel is held to the same bounds against the same reference;
  (b) on a basis: one hot pixel per output channel, so that every dW row is ONE product with 1.0 -- an exact copy of one X row, or
      zeros where the tap leaves the map.  No tolerance.
"""
import functools
from ctypes import c_int

import pytest
import torch
import torch.nn.functional as F

from test_wgrad_forms_cpu import DECONV_FORMS, FORMS, conv_geometry, deconv_geometry, expected_form, form_name

pytestmark = pytest.mark.gpu

CASES = [('conv', r) for r in FORMS] + [('deconv', r) for r in DECONV_FORMS]
IDS = [r[0] for _, r in CASES]
U = 2.0 ** -24                     # unit roundoff of an fp32 addition


def _geometry(kind, row):
    geo = conv_geometry(row) if kind == 'conv' else deconv_geometry(row)
    # the tap whose X gather never leaves the map carries the bias gradient; the transposed conv's taps partition the G pixels
    geo['db_tap'] = -2 if kind == 'deconv' else [i for i, t in enumerate(geo['taps']) if t[2] == 0 and t[3] == 0][0]
    return geo


def _shape_key(geo):
    return (geo['groups'], geo['B'], geo['GH'], geo['GW'], geo['Cout'], geo['XH'], geo['XW'], geo['Cin'], geo['OH'], geo['OW'],
            tuple(geo['taps']), geo['gos'], geo['ss'], geo['db_tap'])


def _valid_pixels(geo):
    """Per tap: the number of (b, oy, ox) whose G and X positions both lie inside their maps = the products in a dW entry."""
    out = []
    for goy, gox, dy, dx, _ in geo['taps']:
        ny = sum(1 for oy in range(geo['OH']) if 0 <= oy * geo['gos'] + goy < geo['GH'] and 0 <= oy * geo['ss'] + dy < geo['XH'])
        nx = sum(1 for ox in range(geo['OW']) if 0 <= ox * geo['gos'] + gox < geo['GW'] and 0 <= ox * geo['ss'] + dx < geo['XW'])
        out.append(geo['B'] * ny * nx)
    return out


@functools.lru_cache(maxsize=None)
def _problem(kind, key, dtype):
    """Operands rounded to the 16-bit type, and in float64 on the CPU: the defining sum, and the same sum over |g| |x| (what the
    rounding error of an entry is relative to).  Made once per shape and shared by every variant / split count of that shape."""
    G, B, GH, GW, Cout, XH, XW, Cin, OH, OW, taps, gos, ss, db_tap = key
    T = len(taps)
    gen = torch.Generator().manual_seed(1000 + G * 131 + B * 17 + Cin + 3 * Cout + 7 * XH + 11 * XW)
    x = torch.randn(G * B, Cin, XH, XW, generator=gen).to(dtype)
    g = torch.randn(G * B, Cout, GH, GW, generator=gen).to(dtype)
    ref = torch.zeros(G, T, Cout, Cin, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for gr in range(G):
        xs, gs = x[gr * B:(gr + 1) * B].double(), g[gr * B:(gr + 1) * B].double()
        for out, xo, go in ((ref, xs, gs), (mag, xs.abs(), gs.abs())):
            if kind == 'conv':
                R = int(round(T ** 0.5))
                pad = -taps[0][2]
                w = torch.zeros(Cout, Cin, R, R, dtype=torch.float64, requires_grad=True)
                (dw,) = torch.autograd.grad(F.conv2d(xo, w, None, stride=ss, padding=pad), w, go)
                out[gr] = dw.permute(2, 3, 0, 1).reshape(T, Cout, Cin)
            else:           # dW[2 py + px][n][c] = sum_{b, y, x} G[b, 2 y + py, 2 x + px, n] X[b, y, x, c]
                for py, px, _, _, wt in taps:
                    out[gr, wt] = torch.einsum('bnyx,bcyx->nc', go[:, :, py::2, px::2], xo)
    gd = g.double().view(G, B, Cout, GH * GW)
    return dict(x=x, g=g, ref=ref, mag=mag, ref_db=gd.sum(dim=(1, 3)), mag_db=gd.abs().sum(dim=(1, 3)))


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _launch(K, geo, g, x, slots_ok=False):
    G, B = geo['groups'], geo['B']
    db = torch.zeros(G, geo['Cout'], dtype=torch.float32, device='cuda')
    dw = K.conv_wgrad(g, x, B, geo['GH'], geo['GW'], geo['Cout'], geo['XH'], geo['XW'], geo['Cin'], geo['OH'], geo['OW'],
                      geo['taps'], len(geo['taps']), gos=geo['gos'], ss=geo['ss'], groups=G, g_gs=B * geo['GH'] * geo['GW'] * geo['Cout'],
                      x_gs=B * geo['XH'] * geo['XW'] * geo['Cin'], splits=geo['splits'], db=db, db_tap=geo['db_tap'], slots_ok=slots_ok)
    return dw, db


def _split_count(K, geo):
    """The K-splits of the launch: what the library answers for the wide kernels.  The narrow kernel has no slots form to ask: for it
    the split rule of the dispatcher, written out (about 512 workgroups of 64 x 64 tiles, at least 256 pixels per split, split
    length a multiple of the 64-pixel K-step)."""
    from bonai_amd import lib as L
    if geo['Cin'] % 128 or geo['Cout'] % 128:
        M, T = geo['B'] * geo['OH'] * geo['OW'], len(geo['taps'])
        splits = geo['splits']
        if splits <= 0:
            tiles = -(-geo['Cout'] // 64) * -(-geo['Cin'] // 64)
            splits = min(max(1, 512 // (tiles * T * geo['groups'])), -(-M // 256))
        pps = -(--(-M // splits) // 64) * 64
        return -(-M // pps)
    A = lambda i: L.arr(c_int, [t[i] for t in geo['taps']])      # noqa: E731
    S = L.load().loft_conv_wgrad_slots(geo['B'], geo['GH'], geo['GW'], geo['Cout'], geo['XH'], geo['XW'], geo['Cin'], geo['OH'],
                                       geo['OW'], geo['gos'], geo['ss'], len(geo['taps']), A(0), A(1), A(2), A(3), A(4), geo['groups'],
                                       geo['splits'], int(geo['variant']))
    assert S >= 1, S
    return S


def _hold_to_bounds(tag, dw, db, P, geo, S):
    """|got - ref| <= 2 n 2^-24 sum|g x| + 1e-30 per entry, n = the products of the entry's sum + the K-splits that are added up (the
    factor 2: the matrix core's multi-term adds need not round to nearest at every step); and the bound of test_conv_wgrad."""
    n_dw = torch.tensor(_valid_pixels(geo), dtype=torch.float64).view(1, -1, 1, 1) + S
    n_db = geo['B'] * geo['GH'] * geo['GW'] + S * (len(geo['taps']) if geo['db_tap'] == -2 else 1)
    e_dw = (dw.double().cpu() - P['ref']).abs()
    e_db = (db.double().cpu() - P['ref_db']).abs()
    b_dw = 2 * n_dw * U * P['mag'] + 1e-30
    b_db = 2 * n_db * U * P['mag_db'] + 1e-30
    r_dw, r_db = (e_dw / b_dw).max().item(), (e_db / b_db).max().item()
    print(f'WGRAD_FORM_RATIO {tag} dw={r_dw:.4f} db={r_db:.4f} max_err={e_dw.max().item():.3e} max_ref={P["ref"].abs().max().item():.3e}')
    assert r_dw <= 1.0, (tag, r_dw)
    assert r_db <= 1.0, (tag, r_db)
    assert e_dw.max().item() < 5e-4 * max(1.0, P['ref'].abs().max().item()), tag
    assert e_db.max().item() < 5e-4 * max(1.0, P['ref_db'].abs().max().item()), tag


@pytest.mark.parametrize('kind,row', CASES, ids=IDS)
def test_full_tensor_parity_with_fp64(kind, row):
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    geo = _geometry(kind, row)
    form = K.conv_wgrad_form(**{k: v for k, v in geo.items() if k != 'db_tap'})
    assert form == expected_form(row), (row[0], form_name(form), row[-1])
    P = _problem(kind, _shape_key(geo), L.act16())
    g, x = _cl(P['g']), _cl(P['x'])
    S = _split_count(K, geo)
    narrow = bool(geo['Cin'] % 128 or geo['Cout'] % 128)
    prev_v, prev_s = K.WGRAD_VARIANT, K.WGRAD_SLOTS
    K.WGRAD_VARIANT = geo['variant']
    try:
        K.WGRAD_SLOTS = False
        dw, db = _launch(K, geo, g, x)
        assert dw.shape == P['ref'].shape
        _hold_to_bounds(f'{row[0]} {row[-1]} atomics', dw, db, P, geo, S)
        if not narrow:
            # split-K slots of the same kernel: plain stores into a buffer nobody zeroed (poisoned: the allocator hands the slots
            # out of this block), every slot written, and their sum held to the SAME reference -- not to the launch above
            poison = torch.full((64 << 20,), float('nan'), device='cuda')
            del poison
            K.WGRAD_SLOTS = True
            slots, db = _launch(K, geo, g, x, slots_ok=True)
            assert slots.dim() == 5 and slots.shape[1] == S and slots.shape[0] == geo['groups'] and slots.shape[2:] == dw.shape[1:], \
                (tuple(slots.shape), S)
            assert torch.isfinite(slots).all()
            _hold_to_bounds(f'{row[0]} {row[-1]} slots', slots.double().sum(1), db, P, geo, S)
    finally:
        K.WGRAD_VARIANT, K.WGRAD_SLOTS = prev_v, prev_s


def _basis_answer(key, xrows, m):
    """G = 1.0 at pixel m[i] (of every group's [B, GH, GW] map) in channel m[i] mod Cout, zero elsewhere; xrows fp32
    [G, B, XH, XW, Cin] -> (dW, db) of the defining sum: dW[wt[t]][m mod Cout] = the X row the tap pairs with that G pixel."""
    G, B, GH, GW, Cout, XH, XW, Cin, OH, OW, taps, gos, ss, _ = key
    n = m % Cout
    b, gy, gx = m // (GH * GW), (m // GW) % GH, m % GW
    want = torch.zeros(G, len(taps), Cout, Cin, dtype=torch.float32, device=xrows.device)
    for goy, gox, dy, dx, wt in taps:
        # G pixel (gy, gx) is the tap's term of output pixel (oy, ox) = ((gy - goy) / gos, (gx - gox) / gos), if there is one
        oy, ox = (gy - goy) // gos, (gx - gox) // gos
        ok = ((gy - goy) % gos == 0) & ((gx - gox) % gos == 0) & (oy >= 0) & (oy < OH) & (ox >= 0) & (ox < OW)
        iy, ix = oy * ss + dy, ox * ss + dx
        ok &= (iy >= 0) & (iy < XH) & (ix >= 0) & (ix < XW)
        rows = xrows[:, b, iy.clamp(0, XH - 1), ix.clamp(0, XW - 1)]          # [G, pixels, Cin]
        want[:, wt, n] = torch.where(ok.view(1, -1, 1), rows, torch.zeros_like(rows))
    hot = torch.zeros(G, Cout, dtype=torch.float32, device=xrows.device)
    hot[:, n] = 1.0
    return want, hot


@pytest.mark.parametrize('kind,row', CASES, ids=IDS)
def test_exact_addressing_on_a_basis(kind, row):
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    geo = _geometry(kind, row)
    form = K.conv_wgrad_form(**{k: v for k, v in geo.items() if k != 'db_tap'})
    assert form == expected_form(row), (row[0], form_name(form), row[-1])
    G, B, GH, GW, Cout, XH, XW, Cin, OH, OW, taps, gos, ss, _ = _shape_key(geo)
    x = _cl(_problem(kind, _shape_key(geo), L.act16())['x'])
    xrows = x.permute(0, 2, 3, 1).reshape(G, B, XH, XW, Cin).float()          # (NHWC in memory; 16 bits -> fp32 is exact)
    NG = B * GH * GW                                                        # G pixels of one group
    g = torch.zeros(G * B, Cout, GH, GW, dtype=L.act16(), device='cuda').contiguous(memory_format=torch.channels_last)
    gpix = g.permute(0, 2, 3, 1).view(G, NG, Cout)                           # the same memory as [group][pixel][channel]
    assert gpix.data_ptr() == g.data_ptr()
    prev_v, prev_s = K.WGRAD_VARIANT, K.WGRAD_SLOTS
    K.WGRAD_VARIANT, K.WGRAD_SLOTS = geo['variant'], False
    try:
        for m0 in range(0, NG, Cout):               # pixels [m0, m0 + Cout) hot, pixel m in channel m mod Cout
            m = torch.arange(m0, min(m0 + Cout, NG), device='cuda')
            g.zero_()
            gpix[:, m, m % Cout] = 1.0
            dw, db = _launch(K, geo, g, x)
            want, hot = _basis_answer(_shape_key(geo), xrows, m)
            assert torch.equal(dw, want), (row[0], m0, (dw != want).nonzero()[:4].tolist())
            assert torch.equal(db, hot), (row[0], m0)
    finally:
        K.WGRAD_VARIANT, K.WGRAD_SLOTS = prev_v, prev_s
