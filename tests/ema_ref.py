"""The reference of the weight EMA (csrc/optim.hip: mte_ema_update, FusedFlatOptimizer(ema_decay > 0)) in NumPy float32.

For the t-th update (t = 1, 2, ...) the decay is d_t = min(decay, (1 + t) / (10 + t)) with the warm-up and d_t = decay without, formed in
double precision; the kernel receives d32 = float32(d_t) and omd32 = float32(1 - double(d32)) and computes e = d32 * e + omd32 * p: two
float32 multiplications and one float32 addition, each rounded once -- NumPy's float32 array arithmetic does exactly that."""
import numpy as np


def decay_pair(t, decay, warmup):
    """(d32, omd32) of the t-th update as np.float32 values"""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + t) / (10.0 + t))
    d32 = np.float32(d)
    return d32, np.float32(1.0 - float(d32))


def update(e, p, d32, omd32):
    """one update of float32 arrays: float32(float32(d32 * e) + float32(omd32 * p))"""
    e, p = np.asarray(e), np.asarray(p)
    assert e.dtype == np.float32 and p.dtype == np.float32
    with np.errstate(all="ignore"):
        out = np.float32(d32) * e + np.float32(omd32) * p
    assert out.dtype == np.float32
    return out


def run(p0, snapshots, decay, warmup, skipped=()):
    """the average after every update: it starts as a copy of p0; snapshots[i] are the weights after step i + 1 (t = i + 1).  A step whose
    number is in ``skipped`` leaves the average untouched, but t advances all the same (the host cannot know a step was skipped)."""
    e = np.array(p0, dtype=np.float32, copy=True)
    for i, p in enumerate(snapshots):
        t = i + 1
        if t in skipped:
            continue
        e = update(e, np.asarray(p, dtype=np.float32), *decay_pair(t, decay, warmup))
    return e
