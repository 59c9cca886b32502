"""The image half of the reference's ``train_transforms`` (packnet_sfm/datasets/transforms.py:17-50) on the device, bit for bit
as PIL / torchvision-on-PIL compute it on the host (csrc/image_prep.hip):

  * ``resize_image_u8``        ``image.crop(borders)`` + ``transforms.Resize(shape, ANTIALIAS)`` (augmentations.py:16-35,385-401)
  * ``draw_color_jitter``      the random draws of ``colorjitter_sample`` (augmentations.py:289-382), same consumption of ``random``
  * ``color_jitter_to_tensor`` the drawn operations + ``ToTensor`` on a uint8 batch, and the ``rgb_original`` copy (:262-287)
  * ``parse_crop_borders``     utils/misc.py:78-140

PNG decoding stays on the host; the tensors handed to these functions are CUDA tensors -- host tensors raise MteError.
"""
import functools
import math
import random

import torch

PRECISION_BITS = 22                                   # PIL ImagingResample, 8 bits per channel
OPS = ('brightness', 'contrast', 'saturation', 'hue')


def _lanczos(x):
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a, b = x * math.pi, (x / 3.0) * math.pi                          # sinc_filter(x) * sinc_filter(x / 3)
        return (math.sin(a) / a) * (math.sin(b) / b)
    return 0.0


@functools.lru_cache(maxsize=64)
def lanczos_coeffs(in_size, out_size):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for LANCZOS, on the host in double precision:
    -> (kk int32 [out, ksize], bounds int32 [out, 2] = (first tap, tap count)) as CPU tensors.  Equal sizes give the identity table
    (one tap of 1 << 22), the form in which the kernel skips a pass like PIL does."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError("sizes must be positive, got {} -> {}".format(in_size, out_size))
    if in_size == out_size:
        kk = torch.full((out_size, 1), 1 << PRECISION_BITS, dtype=torch.int32)
        bounds = torch.stack([torch.arange(out_size, dtype=torch.int32), torch.ones(out_size, dtype=torch.int32)], dim=1)
        return kk, bounds.contiguous()
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    kk, bounds = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        row = [0] * ksize
        for x, v in enumerate(w):
            if ww != 0.0:
                v /= ww
            row[x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        kk.append(row)
        bounds.append((xmin, xmax))
    return torch.tensor(kk, dtype=torch.int32), torch.tensor(bounds, dtype=torch.int32)


@functools.lru_cache(maxsize=64)
def _tables(in_size, out_size, device):
    """the tables of lanczos_coeffs on `device`, bounded like the host cache (KITTI has five frame sizes)"""
    kk, bounds = lanczos_coeffs(in_size, out_size)
    return kk.to(device), bounds.to(device), int(kk.shape[1])


def resize_image_u8(img_u8_hwc, shape, crop=None, two_pass=False):
    """uint8 [h,w,3] CUDA tensor -> uint8 [H,W,3]: PIL ``crop(crop)`` (left, top, right, bottom) + ``resize((W, H), LANCZOS)``.
    two_pass forces the two-launch form with the intermediate image in HBM (same bytes)."""
    from .. import kernels as K
    K._require_gpu(img_u8_hwc)
    if img_u8_hwc.dtype != torch.uint8 or img_u8_hwc.dim() != 3 or img_u8_hwc.shape[2] != 3:
        raise ValueError("expected a uint8 [h,w,3] image, got {} {}".format(img_u8_hwc.dtype, tuple(img_u8_hwc.shape)))
    src = img_u8_hwc.contiguous()
    h, w = int(src.shape[0]), int(src.shape[1])
    left, top, right, bottom = (0, 0, w, h) if crop is None else (int(v) for v in crop)
    if not (0 <= left < right <= w and 0 <= top < bottom <= h):
        raise ValueError("crop window {} does not lie inside the {} x {} image".format(crop, h, w))
    ih, iw = bottom - top, right - left
    H, W = int(shape[0]), int(shape[1])
    kkh, bh, ksh = _tables(iw, W, src.device)
    kkv, bv, ksv = _tables(ih, H, src.device)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=src.device)
    nws = K.lib.mte_image_resample_work_bytes(ih, iw, H, W, int(bool(two_pass)))
    ws = torch.empty(nws, dtype=torch.uint8, device=src.device) if nws else None
    K.lib.mte_image_resample_u8(src.data_ptr(), w * 3, left, top, ih, iw, out.data_ptr(), H, W, kkh.data_ptr(), bh.data_ptr(), ksh,
                                kkv.data_ptr(), bv.data_ptr(), ksv, ws.data_ptr() if nws else None, int(bool(two_pass)), K._stream())
    return out


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def parse_crop_borders(borders, shape):
    """utils/misc.py:78-140: (y, height, x, width) or (y, x) -> (left, top, right, bottom); negative numbers count from the far
    border, floats are a centre given as a fraction of the image with height / width around it."""
    if len(borders) == 0:
        return 0, 0, shape[1], shape[0]
    borders = list(borders)
    if len(borders) == 4:
        borders = [borders[2], borders[0], borders[3], borders[1]]
        if _is_int(borders[0]):
            borders[0] += shape[1] if borders[0] < 0 else 0
            borders[2] += shape[1] if borders[2] <= 0 else borders[0]
        else:
            center_w, half_w = borders[0] * shape[1], borders[2] / 2
            borders[0], borders[2] = int(center_w - half_w), int(center_w + half_w)
        if _is_int(borders[1]):
            borders[1] += shape[0] if borders[1] < 0 else 0
            borders[3] += shape[0] if borders[3] <= 0 else borders[1]
        else:
            center_h, half_h = borders[1] * shape[0], borders[3] / 2
            borders[1], borders[3] = int(center_h - half_h), int(center_h + half_h)
    elif len(borders) == 2:
        borders = [borders[1], borders[0]]
        if _is_int(borders[0]):
            borders = (max(0, borders[0]), max(0, borders[1]), shape[1] + min(0, borders[0]), shape[0] + min(0, borders[1]))
        else:
            center_w, half_w = borders[0] * shape[1], borders[1] / 2
            center_h, half_h = borders[0] * shape[0], borders[1] / 2
            borders = (int(center_w - half_w), int(center_h - half_h), int(center_w + half_w), int(center_h + half_h))
    else:
        raise NotImplementedError('Crop tuple must have 2 or 4 values.')
    assert 0 <= borders[0] < borders[2] <= shape[1] and 0 <= borders[1] < borders[3] <= shape[0], \
        'Crop borders {} are invalid'.format(borders)
    return tuple(borders)


def draw_color_jitter(parameters, rng=random, prob=1.0):
    """The draws of colorjitter_sample + random_color_jitter_transform (augmentations.py:307-380) in the reference's order -- one
    ``random()`` against prob, ``uniform`` for brightness, contrast, saturation, hue, then ``shuffle`` of the four operations -- so that
    after ``random.seed(k)`` the result is the reference's.  -> None (not jittered) or
    {'factors': (brightness, contrast, saturation, hue), 'order': operation indices into OPS in the order they are applied}."""
    if len(parameters) == 0:
        return None
    if len(parameters) > 4 and parameters[4] > 0:
        raise NotImplementedError("the colour matrix (fifth jittering parameter) is not rebuilt")
    if not rng.random() < prob:
        return None
    brightness, contrast, saturation, hue = parameters[:4]
    factors = (rng.uniform(max(0, 1 - brightness), 1 + brightness), rng.uniform(max(0, 1 - contrast), 1 + contrast),
               rng.uniform(max(0, 1 - saturation), 1 + saturation), rng.uniform(-hue, hue))
    order = [0, 1, 2, 3]
    rng.shuffle(order)
    return {'factors': factors, 'order': tuple(order)}


def hue_shift(hue_factor):
    """the uint8 torchvision's adjust_hue adds to the H channel: trunc(hue_factor * 255) mod 256"""
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError("hue_factor {} is not in [-0.5, 0.5]".format(hue_factor))
    return int(hue_factor * 255) % 256


def color_jitter_to_tensor(batch_u8, params_list=None, want_original=False):
    """uint8 [B,H,W,3] CUDA tensor -> float32 [B,3,H,W] = ToTensor(jitter(image)); params_list: one draw_color_jitter result (or
    None = leave alone) per sample, None / empty = plain ToTensor.  want_original: -> (jittered, un-jittered)."""
    from .. import kernels as K
    K._require_gpu(batch_u8)
    if batch_u8.dtype != torch.uint8 or batch_u8.dim() != 4 or batch_u8.shape[3] != 3:
        raise ValueError("expected a uint8 [B,H,W,3] batch, got {} {}".format(batch_u8.dtype, tuple(batch_u8.shape)))
    src = batch_u8.contiguous()
    B, H, W = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    dev = src.device
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    orig = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_original else None
    factors = order = sums = None
    any_contrast = False
    if params_list and any(p is not None for p in params_list):
        if len(params_list) != B:
            raise ValueError("{} parameter sets for a batch of {}".format(len(params_list), B))
        f_rows, o_rows = [], []
        for p in params_list:
            if p is None:
                f_rows.append([0.0] * 4)
                o_rows.append([-1] * 4)
                continue
            f, o = p['factors'], [int(v) for v in p['order']]
            if len(o) > 4 or any(v not in (0, 1, 2, 3) for v in o) or len(set(o)) != len(o):
                raise ValueError("order must name each of the operations 0..3 at most once, got {}".format(p['order']))
            f_rows.append([float(f[0]), float(f[1]), float(f[2]), float(hue_shift(f[3]))])
            o_rows.append(o + [-1] * (4 - len(o)))
            any_contrast = any_contrast or 1 in o
        factors = torch.tensor(f_rows, dtype=torch.float32).to(dev)
        order = torch.tensor(o_rows, dtype=torch.int32).to(dev)
        if any_contrast:
            sums = torch.zeros(B, dtype=torch.int64, device=dev)
    K.lib.mte_color_jitter_u8_to_f32(src.data_ptr(), B, H, W, factors.data_ptr() if factors is not None else None,
                                     order.data_ptr() if order is not None else None, int(any_contrast),
                                     sums.data_ptr() if sums is not None else None, out.data_ptr(),
                                     orig.data_ptr() if orig is not None else None, K._stream())
    return (out, orig) if want_original else out
