"""The contract of bonai_amd/csrc/mask_rle.hip restated in numpy, and the inputs its tests share.

paste_np      the paste rule of csrc/box_codec.h (paste_outside / paste_sample on sigmoid taps), float32, same operation order
translate_np  mask_translate's shift: footprint(y, x) = roof(y + round(dy), x + round(dx)), halves away from zero, 0 outside
counts_np     the run rule: column-major, a run starts where the value differs from the pixel before (m[-1] = 0)
table         the boxes and logits of the tests: one row per situation the encoder has a branch for
kinds         which of the four string / mask kinds a case set must contain a reference string shows
The numpy exp is not the device's expf, so a pixel whose probability lies within an ulp of the threshold may differ from the device's:
this restatement documents the contract and guards the inputs; the GPU tests compare the device with the device.
"""
import numpy as np

f32 = np.float32


def sigmoid_np(logits):
    x = np.asarray(logits, f32)
    return (f32(1) / (f32(1) + np.exp(-x).astype(f32))).astype(f32)


def paste_np(taps, box, h, w, thr):
    """taps: float32 [S,S] probabilities; box (x1, y1, x2, y2) float32 -> bool [h, w]."""
    S = taps.shape[0]
    b = [f32(v) for v in box]
    xs, ys = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    with np.errstate(all='ignore'):
        out_x = (xs.astype(f32) < max(np.floor(b[0]) - f32(1), f32(0))) | (xs.astype(f32) >= min(np.ceil(b[2]) + f32(1), f32(w)))
        out_y = (ys.astype(f32) < max(np.floor(b[1]) - f32(1), f32(0))) | (ys.astype(f32) >= min(np.ceil(b[3]) + f32(1), f32(h)))
        gx = ((xs.astype(f32) + f32(0.5) - b[0]) / (b[2] - b[0]) * f32(2) - f32(1)).astype(f32)
        gy = ((ys.astype(f32) + f32(0.5) - b[1]) / (b[3] - b[1]) * f32(2) - f32(1)).astype(f32)
        gx[np.isinf(gx)] = 0
        gy[np.isinf(gy)] = 0
        sx = (((gx + f32(1)) * f32(S) - f32(1)) * f32(0.5)).astype(f32)
        sy = (((gy + f32(1)) * f32(S) - f32(1)) * f32(0.5)).astype(f32)
        SX, SY = np.meshgrid(sx, sy)
        ok = (SX > -1) & (SX < S) & (SY > -1) & (SY < S)
        fx, fy = np.floor(np.where(ok, SX, 0)).astype(f32), np.floor(np.where(ok, SY, 0)).astype(f32)
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        lx, ly = (np.where(ok, SX, 0) - fx).astype(f32), (np.where(ok, SY, 0) - fy).astype(f32)
        pad = np.zeros((S + 2, S + 2), f32)
        pad[1:-1, 1:-1] = taps

        def at(yy, xx):
            return pad[yy + 1, xx + 1]
        v = (at(y0, x0) * (f32(1) - ly) * (f32(1) - lx) + at(y0, x0 + 1) * (f32(1) - ly) * lx + at(y0 + 1, x0) * ly * (f32(1) - lx)
             + at(y0 + 1, x0 + 1) * ly * lx).astype(f32)
        v = np.where(ok, v, f32(0))
    return (v >= f32(thr)) & ~out_y[:, None] & ~out_x[None, :]


def round_half_away(v):
    return int(np.sign(v) * np.floor(np.abs(np.float32(v)).astype(np.float64) + 0.5))


def translate_np(mask, off):
    h, w = mask.shape
    ox, oy = round_half_away(off[0]), round_half_away(off[1])
    out = np.zeros_like(mask)
    ys, xs = np.arange(h) + oy, np.arange(w) + ox
    vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    out[np.ix_(vy, vx)] = mask[np.ix_(ys[vy], xs[vx])]
    return out


def counts_np(mask):
    """bool [h, w] -> the counts of the column-major runs, the first one the (possibly empty) leading run of zeros."""
    h, w = mask.shape
    m = mask.T.reshape(-1).astype(np.int8)
    change = np.flatnonzero(np.diff(np.concatenate([[0], m])) != 0)
    return np.diff(np.concatenate([[0], change, [h * w]])).tolist()


def table(h, w, S):
    """-> (names, boxes float32 [n,4], logits float32 [n,S,S])."""
    yy, xx = np.meshgrid(np.arange(S, dtype=f32), np.arange(S, dtype=f32), indexing='ij')
    c = f32(S - 1) / 2
    smooth = (4 - 8 * ((yy - c) ** 2 + (xx - c) ** 2) / f32(S / 2) ** 2).astype(f32)        # +4 in the centre, -12 in the corners
    hi, lo = np.full((S, S), 20, f32), np.full((S, S), -20, f32)
    alt = (4 * (1 - 2 * ((yy + xx) % 2))).astype(f32)                                        # +-4 per tap
    mx, my = w // S + 2, h // S + 2          # a margin that puts every image pixel between two taps of a box drawn around it
    rows = [
        ('interior_smooth', [w * .3 + .3, h * .25 + .6, w * .7 + .1, h * .8 - .2], smooth),
        ('cover_hi', [-mx, -my, w + mx, h + my], hi),                        # every pixel set: counts [0, h*w]
        ('image_hi', [0, 0, w, h], hi),
        ('topleft_hi', [-(w * .1 + 2), -(h * .1 + 2), w * .45, h * .5], hi),  # m[0] = 1, negative coordinates
        ('left_smooth', [-(w * .1 + 2), h * .3, w * .3, h * .6], smooth),
        ('top_hi', [w * .3, -(h * .1 + 2), w * .6, h * .3], hi),
        ('right_smooth', [w * .7, h * .3, w * 1.1 + 2, h * .6], smooth),
        ('bottom_hi', [w * .3, h * .7, w * .6, h * 1.1 + 2], hi),
        ('bottomright_hi', [w * .6, h * .6, w + mx, h + my], hi),            # set up to the image's last pixel
        ('stripe_hi', [w * .3, -my, w * .6, h + my], hi),                    # full height: one run through the column boundaries
        ('zero_width', [10.5, 5.25, 10.5, 20], hi),
        ('zero_height', [5, 12.5, 20, 12.5], hi),
        ('zero_both', [w / 2, h / 2, w / 2, h / 2], hi),
        ('interior_lo', [w * .3, h * .3, w * .7, h * .7], lo),               # empty: counts [h*w]
        ('interior_alt', [w * .2 + .3, h * .2 + .4, w * .8, h * .85], alt),  # many short runs
        ('bottom_alt', [w * .1, h * .5, w * .5, h + my], alt),
    ]
    return [r[0] for r in rows], np.array([r[1] for r in rows], f32), np.stack([r[2] for r in rows]).astype(f32)


BIG = ('interior_smooth', 'cover_hi', 'topleft_hi', 'interior_alt')


def big_table(S, size=1024):
    """The four detections of the 1024^2 case: rows of the table, the interior ones moved to the right half so that their leading runs
    of zeros are about 5e5 pixels long (a count of four characters)."""
    names, boxes, logits = table(size, size, S)
    keep = [names.index(n) for n in BIG]
    boxes = boxes[keep].copy()
    boxes[0] = [size * .49 + .3, size * .25 + .6, size * .7 + .1, size * .8 - .2]
    boxes[3] = [size * .47 + .3, size * .2 + .4, size * .8, size * .85]
    return list(BIG), boxes, logits[keep]


def string_fields(s):
    """compressed string -> [(value as written, number of characters)] per count (cocoapi rleFrString, before the differences)."""
    out, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            ch = s[p] - 48
            x |= (ch & 0x1f) << (5 * k)
            more = bool(ch & 0x20)
            p += 1
            k += 1
            if not more and (ch & 0x10):
                x |= -1 << (5 * k)
        out.append((x, k))
    return out


def kinds(s, mask):
    """The kinds of a string and its bool [h, w] mask among: leading count 0, a run through a column boundary, a count of at least
    four characters, a negative difference."""
    f = string_fields(s)
    k = set()
    if f[0][0] == 0:
        k.add('leading0')
    if (mask[-1, :-1] & mask[0, 1:]).any():
        k.add('column_boundary')
    if any(n >= 4 for _, n in f):
        k.add('four_chars')
    if any(x < 0 for x, _ in f[3:]):
        k.add('negative_diff')
    return k


ALL_KINDS = {'leading0', 'column_boundary', 'four_chars', 'negative_diff'}
