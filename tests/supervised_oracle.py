"""CPU restatement of the supervised losses of SupervisedLoss (packnet_sfm/losses/supervised_loss.py:13-216, utils/image.py:122-220,
utils/depth.py depth2inv) and of the nearest upsample of upsample_depth_maps (models/model_utils.py:154-176), in plain PyTorch: the
yardstick of tests/test_supervised_loss_cpu.py and tests/test_gpu_supervised_loss.py."""
import torch
import torch.nn.functional as F

SUFFIXES = ("l1", "mse", "berhu", "silog", "abs_rel")
ACCEPTED = tuple(p + s for s in SUFFIXES for p in ("sparse-", "") if (p, s) != ("", "berhu"))   # all but dense berhu


def parse(method):
    """-> (suffix, sparse) as get_loss_func picks the loss: the first suffix the string ends with."""
    for s in SUFFIXES:
        if method.endswith(s):
            return s, method.startswith("sparse")
    raise ValueError("Unknown supervised loss {}".format(method))


def depth2inv(depth):
    inv = 1.0 / depth.clamp(min=1e-6)
    return torch.where(depth > 0, inv, torch.zeros_like(inv))


def nearest(img, shape):
    """F.interpolate(mode='nearest'), skipped at equal size (interpolate_image / match_scales)."""
    if tuple(img.shape[-2:]) == tuple(shape):
        return img
    return F.interpolate(img, size=tuple(shape), mode="nearest")


def berhu(x, y, threshold=0.2):
    c = threshold * torch.max(x - y)
    d = (x - y).abs()
    d2 = d[(d > c).detach()] ** 2
    return torch.cat((d.flatten(), d2)).mean()


def silog(x, y, ratio=10, ratio2=0.85):
    l = torch.log(x * ratio) - torch.log(y * ratio)
    return torch.sqrt(torch.mean(l ** 2) - ratio2 * (l.mean() ** 2)) * ratio


LOSSES = {
    "l1": lambda x, y: (x - y).abs().mean(),
    "mse": lambda x, y: ((x - y) ** 2).mean(),
    "berhu": berhu,
    "silog": silog,
    "abs_rel": lambda x, y: torch.mean(torch.abs(x - y) / x),
}


def supervised_loss(method, n, inv_depths, depth):
    """sum_s f(inv_s + 1e-5, nearest(depth2inv(depth)) at scale s) / n, sparse methods over the pixels with gt > 0."""
    suffix, sparse = parse(method)
    gt = depth2inv(depth)
    total = 0
    for s in range(n):
        x, y = inv_depths[s], nearest(gt, inv_depths[s].shape[-2:])
        if sparse:
            m = (y > 0).detach()
            x, y = x[m], y[m]
        total = total + LOSSES[suffix](x + 1e-5, y)
    return total / n


def upsample(inv_depths):
    """every map nearest-upsampled to the size of scale 0"""
    return [nearest(t, inv_depths[0].shape[-2:]) for t in inv_depths]
