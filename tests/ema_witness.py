"""Witness of the parameter EMA (nerf/ema.py, csrc/ema.hip) in numpy, no torch: torch_ema 0.3's update rule and decay schedule
restated from its documented behaviour.

    n  = number of updates so far, this one included (1, 2, ...)
    d  = min(decay, (1 + n) / (10 + n))        in double; d = decay with use_num_updates=False
    c  = float32(1.0 - d)
    t  = s - p;  t = t * c;  s = s - t         three fp32 roundings per element, nothing contracted

numpy rounds every fp32 operation on its own, so `update` below is that rule exactly."""
import numpy as np


def decay_at(decay, n, use_num_updates=True):
    """the decay of update number n (counted from 1), a Python double"""
    return min(float(decay), (1 + n) / (10 + n)) if use_num_updates else float(decay)


def coefficient(decay, n, use_num_updates=True):
    return np.float32(1.0 - decay_at(decay, n, use_num_updates))


def update(shadow, param, c):
    """the new shadow (a new fp32 array) after one update toward `param` with coefficient c = float32(1 - d)"""
    s, p, c = np.asarray(shadow, dtype=np.float32), np.asarray(param, dtype=np.float32), np.float32(c)
    with np.errstate(all="ignore"):
        t = np.subtract(s, p, dtype=np.float32)
        t = np.multiply(t, c, dtype=np.float32)
        return np.subtract(s, t, dtype=np.float32)


def contracted_update(shadow, param, c):
    """what a fused multiply-subtract would give instead (s - t*c with ONE rounding): the form the kernels must NOT compute"""
    s, p = np.asarray(shadow, dtype=np.float32), np.asarray(param, dtype=np.float32)
    t = np.subtract(s, p, dtype=np.float32)
    return (s.astype(np.float64) - t.astype(np.float64) * np.float64(np.float32(c))).astype(np.float32)


class Witness:
    """shadows of a list of arrays, seeded from their values, update count 0"""

    def __init__(self, params, decay, use_num_updates=True):
        self.decay, self.use_num_updates = float(decay), bool(use_num_updates)
        self.shadows = [np.array(p, dtype=np.float32, copy=True) for p in params]
        self.num_updates = 0

    def update(self, params):
        self.num_updates += 1
        c = coefficient(self.decay, self.num_updates, self.use_num_updates)
        self.shadows = [update(s, p, c) for s, p in zip(self.shadows, params)]
        return c


def same_bits(a, b):
    """bit-for-bit equality of two fp32 arrays (-0 != +0, NaNs compare by payload)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
