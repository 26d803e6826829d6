"""numpy form of a free-surface gauge's record (include/mph_gpu.h mph_gauge_*), from mph_get data:
the reference of tests/test_gpu_gauge.py and tests/test_gpu_gauge_driver.py.

A gauge reads the sorted set of the sampled step -- the wrapped positions before that step's
motion -- so the reference takes get("Position") from before the step and wraps it as
move_and_wrap does, bit for bit for a fluid particle: x = Mod(x - lo, w) + lo.
"""
import math

import numpy as np

EMPTY = (0.0, -np.inf, np.inf, 0.0)


def mod(x, w):
    return x - w * np.floor(x / w)   # the reference's Mod (main.cpp:98)


def nbins(cfg, axis):
    return int(math.ceil((cfg.domain_max[axis] - cfg.domain_min[axis]) / cfg.particle_spacing))


def wrapped(cfg, pos_before):
    lo = np.array([cfg.domain_min[d] for d in range(3)])
    w = np.array([cfg.domain_max[d] - cfg.domain_min[d] for d in range(3)])
    return mod(pos_before - lo, w) + lo, lo, w


def record(cfg, x, lo, w, T, point, axis, h, guard=False):
    """({COUNT, TOP, BOTTOM, WET}, the contributing particles' wrapped positions) of the line through
    `point` along `axis` over the fluid particles of the wrapped set x (wrapped(cfg, before)).
    guard: assert that no fluid particle lies within 1e-9 of the gauge's cylinder."""
    p = mod(np.asarray(point, float) - lo, w) + lo
    d = mod(x - p + 0.5 * w, w) - 0.5 * w
    across = [a for a in range(cfg.dim) if a != axis]
    r2 = d[:, across[0]] * d[:, across[0]]
    if len(across) == 2:
        r2 = r2 + d[:, across[1]] * d[:, across[1]]
    r = np.sqrt(r2)
    fl = T < 2
    if guard:
        assert not (fl & (np.abs(r - h) < 1e-9)).any(), "a fluid particle on the gauge's cylinder"
    sel = fl & (r < h)
    if not sel.any():
        return EMPTY, x[sel]
    xa = x[sel, axis]
    b = np.floor((xa - cfg.domain_min[axis]) / cfg.particle_spacing).astype(np.int64)
    b = np.minimum(np.maximum(b, 0), nbins(cfg, axis) - 1)
    return (float(sel.sum()), float(xa.max()), float(xa.min()), float(len(np.unique(b)))), x[sel]
