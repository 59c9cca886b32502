"""The reference's evaluation transforms (packnet_sfm/datasets/transforms.py:53-125) on the device:

  * ``validation_sample``  validation_transforms: crop of the network's inputs, every input resized to the cropped frame rounded down to a
                           multiple of 32, ToTensor
  * ``test_sample``        test_transforms: the same crop, rgb to ``image_shape`` when one is given, input_depth with the nearest resize
  * ``resize_linear_u8``   cv2.resize(uint8 map, (W, H)) with INTER_LINEAR (fixed point; area average at exactly 2x)   csrc/eval_prep.hip
  * ``resize_nearest_f32`` cv2.resize(float map, (W, H), INTER_NEAREST), the reference's resize_depth                   csrc/eval_prep.hip

Both kernels are PARITY-UNPINNED restatements of OpenCV's published algorithms (no OpenCV where this was written); they are pinned bit for
bit to the NumPy statement in tests/eval_prep_ref.py.  The LANCZOS resize of the frame and resize_depth_preserve are the pinned kernels of
image_prep.py / kitti_edges.py.  A sample holds device tensors as the file readers leave them: rgb uint8 [h,w,3], depth / input_depth float32
[h,w], edge / edge_1..5 / rgb_edge uint8 (PNG) or float32 (.npy) [h,w]; host tensors raise MteError."""
import torch

from . import image_prep as ip

CROPPED_KEYS = ('rgb', 'input_depth', 'rgb_edge')        # crop_sample_input, augmentations.py:447-492: what goes INTO the network
EDGE_SCALES = 5


def _maps(t, dtype):
    from .. import kernels as K
    K._require_gpu(t)
    if t.dtype != dtype:
        raise ValueError("expected {} maps, got {}".format(dtype, t.dtype))
    if t.dim() not in (2, 3):
        raise ValueError("expected [h,w] or [B,h,w], got {}".format(tuple(t.shape)))
    return (t.unsqueeze(0) if t.dim() == 2 else t).contiguous(), t.dim() == 2


def resize_linear_u8(maps_u8, shape):
    """uint8 [h,w] / [B,h,w] CUDA tensor -> uint8 [H,W] / [B,H,W] like ``cv2.resize(map, (W, H))`` (INTER_LINEAR, the default)."""
    from .. import kernels as K
    src, squeeze = _maps(maps_u8, torch.uint8)
    B, h, w = src.shape
    H, W = int(shape[0]), int(shape[1])
    out = torch.empty((B, H, W), dtype=torch.uint8, device=src.device)
    K.lib.mte_resize_linear_u8(src.data_ptr(), B, h, w, out.data_ptr(), H, W, K._stream())
    return out[0] if squeeze else out


def resize_nearest_f32(maps, shape):
    """float32 [h,w] / [B,h,w] CUDA tensor -> [H,W] / [B,H,W] like ``cv2.resize(map, (W, H), interpolation=cv2.INTER_NEAREST)``."""
    from .. import kernels as K
    src, squeeze = _maps(maps, torch.float32)
    B, h, w = src.shape
    H, W = int(shape[0]), int(shape[1])
    out = torch.empty((B, H, W), dtype=torch.float32, device=src.device)
    K.lib.mte_resize_nearest_f32(src.data_ptr(), B, h, w, out.data_ptr(), H, W, K._stream())
    return out[0] if squeeze else out


def _to_tensor_rgb(frame_u8):
    return ip.color_jitter_to_tensor(frame_u8.unsqueeze(0))[0]              # ToTensor: [3,H,W] float32, u8 / 255


def _to_tensor_map(m):
    """ToTensor on a single-channel array: uint8 -> float32 / 255, float unchanged; [1,H,W]"""
    if m.dtype == torch.uint8:
        from .kitti_edges import _u8
        from .. import kernels as K
        src = _u8(m)
        out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
        # float(double(v) / 255.0) equals ToTensor's float32(v) / 255 for all 256 byte values (tests/test_eval_prep_ref.py)
        K.lib.mte_edge_target_from_u8(src.data_ptr(), out.data_ptr(), src.numel(), K._stream())
        return out.unsqueeze(0)
    return m.float().unsqueeze(0)


def _resize_edge(m, shape):
    if m.dtype == torch.uint8:
        return resize_linear_u8(m, shape)
    from ..utils.edge import resize_linear
    return resize_linear(m, shape)                                          # float (.npy) maps: the float bilinear, no scaling


def crop_sample_input(sample, crop_eval_borders):
    """-> (sample with 'input_depth' / 'rgb_edge' cropped, the (left, top, right, bottom) window of 'rgb').  The frame itself is cropped by
    the resize that follows (resize_image_u8 reads the window), so it is returned whole."""
    h, w = int(sample['rgb'].shape[0]), int(sample['rgb'].shape[1])
    if len(crop_eval_borders) == 0:
        return dict(sample), None
    borders = ip.parse_crop_borders(tuple(crop_eval_borders), (h, w))
    out = dict(sample)
    for key in CROPPED_KEYS[1:]:
        if key in out:
            out[key] = out[key][borders[1]:borders[3], borders[0]:borders[2]].contiguous()
    return out, borders


def _frame(rgb, shape, borders):
    h, w = (int(rgb.shape[0]), int(rgb.shape[1])) if borders is None else (borders[3] - borders[1], borders[2] - borders[0])
    if borders is None and (h, w) == tuple(shape):
        return rgb.contiguous()
    return ip.resize_image_u8(rgb, shape, crop=borders)


def validation_sample(sample, crop_eval_borders=()):
    """transforms.py:53-97.  'depth', 'edge' and the coarser edge scales keep their frame before the resize; 'depth' keeps its native size
    (the depth metrics scale the prediction to it)."""
    s, borders = crop_sample_input(sample, crop_eval_borders)
    h, w = (int(s['rgb'].shape[0]), int(s['rgb'].shape[1])) if borders is None else (borders[3] - borders[1], borders[2] - borders[0])
    H, W = h - h % 32, w - w % 32
    if H <= 0 or W <= 0:
        raise ValueError("the cropped frame {} x {} is smaller than 32 pixels in one axis".format(h, w))
    out = {k: v for k, v in s.items() if not torch.is_tensor(v)}
    out['rgb'] = _to_tensor_rgb(_frame(s['rgb'], (H, W), borders))
    if 'input_depth' in s:
        from .kitti_edges import resize_depth_preserve
        out['input_depth'] = resize_depth_preserve(s['input_depth'], (H, W)).unsqueeze(0)
    if 'depth' in s:
        out['depth'] = s['depth'].float().unsqueeze(0)
    shapes = [('edge', (H, W)), ('rgb_edge', (H, W))] + [('edge_%d' % i, (int(H / 2 ** i), int(W / 2 ** i))) for i in range(1, EDGE_SCALES + 1)]
    for key, shape in shapes:
        if key in s:
            out[key] = _to_tensor_map(_resize_edge(s[key], shape))
    return out


def test_sample(sample, image_shape=(), crop_eval_borders=()):
    """transforms.py:101-125: only rgb and input_depth are resized, and only when an image_shape is given."""
    s, borders = crop_sample_input(sample, crop_eval_borders)
    out = {k: v for k, v in s.items() if not torch.is_tensor(v)}
    if len(image_shape) > 0:
        shape = (int(image_shape[0]), int(image_shape[1]))
        out['rgb'] = _to_tensor_rgb(_frame(s['rgb'], shape, borders))
        if 'input_depth' in s:
            out['input_depth'] = resize_nearest_f32(s['input_depth'].float(), shape).unsqueeze(0)
    else:
        rgb = s['rgb'] if borders is None else s['rgb'][borders[1]:borders[3], borders[0]:borders[2]]
        out['rgb'] = _to_tensor_rgb(rgb.contiguous())
        if 'input_depth' in s:
            out['input_depth'] = s['input_depth'].float().unsqueeze(0)
    if 'depth' in s:
        out['depth'] = s['depth'].float().unsqueeze(0)
    for key in ('edge', 'rgb_edge'):
        if key in s:
            out[key] = _to_tensor_map(s[key])
    return out


test_sample.__test__ = False
