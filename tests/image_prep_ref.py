"""numpy restatement of the 8-bit image half of the reference's train_transforms, as PIL (ImagingResample, ImagingBlend, Convert.c) and
torchvision's PIL backend compute it: crop + antialiased LANCZOS resize, the four colour-jitter operations, ToTensor.  The CPU tests pin it
bit for bit against PIL and against the fixtures produced by the reference; the GPU tests compare the HIP kernels with it."""
import math

import numpy as np

PRECISION_BITS = 22
OPS = ("brightness", "contrast", "saturation", "hue")


def _lanczos(x):
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a, b = x * math.pi, (x / 3.0) * math.pi
        return (math.sin(a) / a) * (math.sin(b) / b)
    return 0.0


def precompute_coeffs(in_size, out_size):
    """PIL precompute_coeffs + normalize_coeffs_8bpc for the LANCZOS filter -> (int32 kk[out][ksize], int32 bounds[out][2])."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(a, kk, bounds):
    """one resample pass along axis 1 of uint8 [n, in, c] -> uint8 [n, out, c]; 32-bit accumulators like PIL"""
    out = np.empty((a.shape[0], kk.shape[0], a.shape[2]), np.uint8)
    src = a.astype(np.int32)
    for xx in range(kk.shape[0]):
        xmin, cnt = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full((a.shape[0], a.shape[2]), 1 << (PRECISION_BITS - 1), np.int32)
        for k in range(cnt):
            acc = acc + src[:, xmin + k, :] * kk[xx, k]
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8(img, shape, crop=None):
    """Image.crop(borders) + Image.resize((W, H), LANCZOS) of uint8 [h,w,3]; crop = (left, top, right, bottom)."""
    if crop is not None:
        img = img[crop[1]:crop[3], crop[0]:crop[2]]
    H, W = shape
    if img.shape[1] != W:
        img = _pass(img, *precompute_coeffs(img.shape[1], W))
    if img.shape[0] != H:
        img = _pass(img.transpose(1, 0, 2), *precompute_coeffs(img.shape[0], H)).transpose(1, 0, 2)
    return np.ascontiguousarray(img)


def luma(img):
    i = img.astype(np.int64)
    return ((19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, factor):
    """Image.blend(degenerate, image, factor) on uint8 arrays (float32 arithmetic, truncation; clipping outside [0, 1])"""
    f = np.float32(factor)
    d, i = deg.astype(np.float32), img.astype(np.float32)
    t = d + f * (i - d)
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def adjust_brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast_mean(img):
    L = luma(img)
    return int(int(L.sum(dtype=np.int64)) / L.size + 0.5)


def adjust_contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def adjust_saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, f)


def rgb_to_hsv(img):
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    f32 = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(f32)
        s = cr / maxc.astype(f32)
        rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
        rd, gd, bd = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
        h = np.where(r == maxc, (bc - gc).astype(np.float64), np.where(g == maxc, 2.0 + rd - bd, 4.0 + gd - rd)).astype(f32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)
        H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H, S = np.where(grey, 0, H), np.where(grey, 0, S)
    return np.stack([H, S, maxc], axis=-1).astype(np.uint8)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb(hsv):
    f32 = np.float32
    h, s, v = (hsv[..., c] for c in range(3))
    hf = h.astype(f32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int32)
    f = (hf - i.astype(f32).astype(np.float64)).astype(f32)
    fs = (s.astype(f32).astype(np.float64) / 255.0).astype(f32)
    vd = v.astype(np.float64)
    fsd, fd = fs.astype(np.float64), f.astype(np.float64)
    p = np.clip(_round_half_away(vd * (1.0 - fsd)), 0, 255).astype(np.uint8)
    q = np.clip(_round_half_away(vd * (1.0 - (fs * f).astype(np.float64))), 0, 255).astype(np.uint8)
    t = np.clip(_round_half_away(vd * (1.0 - fsd * (1.0 - fd))), 0, 255).astype(np.uint8)
    i = i % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.empty(hsv.shape, np.uint8)
    for c in range(3):
        out[..., c] = np.select([i == k for k in range(6)], [table[k][c] for k in range(6)])
    grey = s == 0
    for c in range(3):
        out[..., c] = np.where(grey, v, out[..., c])
    return out


def hue_shift(hue_factor):
    """the uint8 added to the H channel by torchvision's adjust_hue: trunc(hue_factor * 255) mod 256"""
    return int(hue_factor * 255) % 256


def adjust_hue(img, hue_factor):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(hue_factor)) % 256
    return hsv_to_rgb(hsv)


ADJUST = (adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue)


def color_jitter(img, factors, order):
    """factors = (brightness, contrast, saturation, hue), order = the operation indices in the order they are applied"""
    for op in order:
        img = ADJUST[op](img, factors[op])
    return img


def to_tensor(img):
    return np.ascontiguousarray((img.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))
