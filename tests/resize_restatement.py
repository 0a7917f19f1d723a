"""The two resampling rules of bonai_amd/csrc/resize.hip and the composition around them, restated in plain numpy and Python loops,
sharing no code with bonai_amd (kernels.resize_tables included).

linear_taps     per output index of one axis: (first tap, a0, a1) -- the sample position in float64, cast to float32, floor,
                the two border cases, coefficients rint(. * 2048) half to even
resize_linear   uint8 [H,W,C] -> uint8 [Hd,Wd,C]: horizontal pass S = v[s] * a0 + v[s + 1] * a1, vertical pass
                (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2; the 2 x 2 mean when the source is exactly twice the target
nearest_index   per output index of one axis: min(floor(d * (1.0 / (D / S))), S - 1) in float64
resize_nearest  uint8 [K,H,W] -> uint8 [K,Hd,Wd]
d4              an element of the square's symmetries on axes (ay, ax): out[y][x] = in[r][c], (r, c) = T ? (x', y') : (y', x'),
                x' = FX ? W - 1 - x : x, y' = FY ? H - 1 - y : y, with index arrays built in loops
image_prep      Resize, element, Normalize (float32 subtract, float32 divide), zero Pad, HWC -> CHW
mask_prep       Resize (nearest), element, zero Pad
"""
import math

import numpy as np

f32 = np.float32
T, FX, FY = 1, 2, 4


def linear_taps(S, D):
    taps = []
    scale = float(S) / float(D)
    for d in range(D):
        fx = f32((d + 0.5) * scale - 0.5)
        sx = int(math.floor(float(fx)))
        fx = f32(fx - f32(sx))
        if sx < 0:
            sx, fx = 0, f32(0)
        if sx >= S - 1:
            sx, fx = S - 1, f32(0)
        a0 = int(np.rint(f32(f32(1) - fx) * f32(2048)))
        a1 = int(np.rint(fx * f32(2048)))
        taps.append((sx, a0, a1))
    return taps


def resize_linear(img, Hd, Wd):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    Hs, Ws, C = img.shape
    v = img.astype(np.int32)
    out = np.zeros((Hd, Wd, C), np.int32)
    if Ws == 2 * Wd and Hs == 2 * Hd:
        for y in range(Hd):
            for x in range(Wd):
                out[y, x] = (v[2 * y, 2 * x] + v[2 * y, 2 * x + 1] + v[2 * y + 1, 2 * x] + v[2 * y + 1, 2 * x + 1] + 2) >> 2
        return out.astype(np.uint8)
    xt, yt = linear_taps(Ws, Wd), linear_taps(Hs, Hd)
    for y, (sy, b0, b1) in enumerate(yt):
        sy1 = min(sy + 1, Hs - 1)
        for x, (sx, a0, a1) in enumerate(xt):
            sx1 = min(sx + 1, Ws - 1)
            S0 = v[sy, sx] * a0 + v[sy, sx1] * a1
            S1 = v[sy1, sx] * a0 + v[sy1, sx1] * a1
            out[y, x] = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def nearest_index(S, D):
    return [min(int(math.floor(d * (1.0 / (D / S)))), S - 1) for d in range(D)]


def resize_nearest(masks, Hd, Wd):
    masks = np.asarray(masks)
    K, Hs, Ws = masks.shape
    yi, xi = nearest_index(Hs, Hd), nearest_index(Ws, Wd)
    out = np.zeros((K, Hd, Wd), masks.dtype)
    for y in range(Hd):
        for x in range(Wd):
            out[:, y, x] = masks[:, yi[y], xi[x]]
    return out


def d4(a, elem, ay=0, ax=1):
    a = np.moveaxis(np.asarray(a), (ay, ax), (0, 1))
    Hi, Wi = a.shape[:2]
    H, W = (Wi, Hi) if elem & T else (Hi, Wi)
    rr, cc = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            xp = W - 1 - x if elem & FX else x
            yp = H - 1 - y if elem & FY else y
            rr[y, x], cc[y, x] = (xp, yp) if elem & T else (yp, xp)
    return np.moveaxis(a[rr, cc], (0, 1), (ay, ax))


def image_prep(img, size, pad_shape, elem=0, keep=False, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """img uint8 [Hs,Ws,3] -> float32 [3,Hp,Wp].  keep: channel c of the output is channel c of the input, else reversed."""
    view = d4(resize_linear(img, size[0], size[1]), elem)
    if not keep:
        view = view[:, :, ::-1]
    x = (view.astype(f32) - np.asarray(mean, f32)) / np.asarray(std, f32)
    assert x.dtype == f32
    out = np.zeros((3, pad_shape[0], pad_shape[1]), f32)
    out[:, :view.shape[0], :view.shape[1]] = x.transpose(2, 0, 1)
    return out


def mask_prep(masks, size, pad_shape, elem=0):
    """masks uint8 [K,Hs,Ws] -> uint8 [K,Hp,Wp]."""
    view = d4(resize_nearest(masks, size[0], size[1]), elem, 1, 2)
    out = np.zeros((view.shape[0], pad_shape[0], pad_shape[1]), np.uint8)
    out[:, :view.shape[1], :view.shape[2]] = view
    return out
