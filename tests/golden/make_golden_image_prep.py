"""Golden vectors of the image half of train_transforms (packnet_sfm/datasets/transforms.py:17-50): runs the REAL reference's
``resize_image``, ``crop_sample``, ``parse_crop_borders``, ``colorjitter_sample`` and ``to_tensor`` on small random and smooth frames and
stores inputs, the drawn jitter parameters and outputs in tests/golden/image_prep.npz.  Development container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_prep.py

torchvision is not installed there, so ``torchvision.transforms`` is a stub written with PIL (Resize, Lambda, Compose, ToTensor and the four
functional.adjust_* as torchvision's PIL backend defines them; the hue wrapper adds trunc(hue_factor * 255) mod 256 to the H channel).  The
stub records every adjust_* call, which is how the parameters and the operation order the reference drew are read back."""
import json
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

CALLS = []
OPS = ("brightness", "contrast", "saturation", "hue")


def _install_torchvision_stub():
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    fn = types.ModuleType("torchvision.transforms.functional")

    class Resize:
        def __init__(self, size, interpolation=Image.BILINEAR):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            return img.resize(tuple(self.size[::-1]), self.interpolation)

    class Lambda:
        def __init__(self, lambd):
            self.lambd = lambd

        def __call__(self, img):
            return self.lambd(img)

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, img):
            for t in self.transforms:
                img = t(img)
            return img

    class ToTensor:
        def __call__(self, pic):
            if isinstance(pic, np.ndarray):
                a = pic[:, :, None] if pic.ndim == 2 else pic
                t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
                return t.float().div(255) if t.dtype == torch.uint8 else t
            return torch.from_numpy(np.asarray(pic, dtype=np.uint8).copy()).permute(2, 0, 1).contiguous().float().div(255)

    def adjust_brightness(img, f):
        CALLS.append((0, f))
        return ImageEnhance.Brightness(img).enhance(f)

    def adjust_contrast(img, f):
        CALLS.append((1, f))
        return ImageEnhance.Contrast(img).enhance(f)

    def adjust_saturation(img, f):
        CALLS.append((2, f))
        return ImageEnhance.Color(img).enhance(f)

    def adjust_hue(img, f):
        CALLS.append((3, f))
        assert -0.5 <= f <= 0.5
        h, s, v = img.convert("HSV").split()
        np_h = (np.array(h, dtype=np.int32) + int(f * 255) % 256) % 256
        h = Image.fromarray(np_h.astype(np.uint8), "L")
        return Image.merge("HSV", (h, s, v)).convert("RGB")

    fn.adjust_brightness, fn.adjust_contrast, fn.adjust_saturation, fn.adjust_hue = adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue
    tr.Resize, tr.Lambda, tr.Compose, tr.ToTensor, tr.functional = Resize, Lambda, Compose, ToTensor, fn
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"], sys.modules["torchvision.transforms.functional"] = tv, tr, fn


def smooth(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    ch = [127.5 + 127.5 * np.sin(x / (3.0 + 5 * g.random()) + y / (4.0 + 6 * g.random()) + 6 * g.random()) for _ in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def main():
    _install_torchvision_stub()
    ref_import.install_stubs()
    from packnet_code.packnet_sfm.datasets import augmentations as A
    from packnet_code.packnet_sfm.utils.misc import parse_crop_borders
    g = np.random.default_rng(7)
    out = {}
    # resize_image
    frames = {"rand": g.integers(0, 256, (97, 131, 3), dtype=np.uint8), "smooth": smooth(97, 131, 1),
              "mixed": g.integers(0, 256, (50, 70, 3), dtype=np.uint8), "skip": g.integers(0, 256, (64, 64, 3), dtype=np.uint8)}
    shapes = {"rand": (64, 192), "smooth": (64, 192), "mixed": (120, 33), "skip": (64, 100)}
    for name, a in frames.items():
        out["resize_%s_in" % name] = a
        out["resize_%s_shape" % name] = np.array(shapes[name])
        out["resize_%s_out" % name] = np.asarray(A.resize_image(Image.fromarray(a), shapes[name]))
    # parse_crop_borders + crop_sample + resize_sample's image part
    cases = []
    for borders, shape in [((10, 60, 7, 100), (97, 131)), ((-50, 0, -100, 0), (97, 131)), ((0.5, 40, 0.5, 64), (97, 131)), ((5, 9), (97, 131)),
                           ((-5, -9), (97, 131)), ((40, 0.5), (97, 131)), ((0, 0, 0, 0), (375, 1242)), ((-352, 0, 0.5, 1216), (375, 1242)), ((), (97, 131))]:
        cases.append({"borders": list(borders), "shape": list(shape), "result": list(parse_crop_borders(borders, shape))})
    out["crop_cases"] = np.array(json.dumps(cases))
    depth = (g.random((97, 131)) < 0.2) * (1 + 80 * g.random((97, 131)))
    edge = ((g.random((97, 131)) < 0.1) * 255).astype(np.uint8)
    out["crop_depth_in"], out["crop_edge_in"] = depth, edge
    for i, c in enumerate(cases[:3]):
        sample = {"rgb": Image.fromarray(frames["rand"]), "depth": depth.copy(), "edge": edge.copy()}
        sample = A.crop_sample(sample, tuple(c["result"]))
        out["crop%d_borders" % i] = np.array(c["result"])
        out["crop%d_rgb" % i] = np.asarray(sample["rgb"])
        out["crop%d_depth" % i], out["crop%d_edge" % i] = sample["depth"], sample["edge"]
        out["crop%d_rgb_resized" % i] = np.asarray(A.resize_image(sample["rgb"], (64, 192)))
    # colorjitter_sample after random.seed(k) + to_tensor
    jit = {"rand": g.integers(0, 256, (48, 64, 3), dtype=np.uint8), "smooth": smooth(48, 64, 2)}
    params = (0.2, 0.2, 0.2, 0.05)
    seeds = list(range(16))
    out["jitter_params"], out["jitter_seeds"] = np.array(params), np.array(seeds)
    for name, a in jit.items():
        out["jitter_%s_in" % name] = a
        out["jitter_%s_tensor" % name] = A.to_tensor(Image.fromarray(a)).numpy()
    factors, orders = [], []
    for k in seeds:
        for name, a in jit.items():
            random.seed(k)
            del CALLS[:]
            sample = A.colorjitter_sample(A.duplicate_sample({"rgb": Image.fromarray(a)}), params)
            out["jitter_%s_seed%d" % (name, k)] = np.asarray(sample["rgb"])
            assert np.array_equal(np.asarray(sample["rgb_original"]), a)
            if name == "rand":
                f = [0.0] * 4
                for op, v in CALLS:
                    f[op] = v
                factors.append(f)
                orders.append([op for op, _ in CALLS])
                if k < 4:
                    out["jitter_rand_seed%d_tensor" % k] = A.to_tensor(sample["rgb"]).numpy()
    out["jitter_factors"], out["jitter_orders"] = np.array(factors, dtype=np.float64), np.array(orders, dtype=np.int32)
    print("contrast position per seed:", [o.index(1) for o in orders])
    path = os.path.join(HERE, "image_prep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
