"""The weight average's update rule restated in numpy float32 (include/avid_hip.h, "Weight averaging"): what the averaging
kernels are held to bit for bit.

    e = e + w * (p - e)       the difference, the product and the sum each rounded to float32 on its own
    w = float32(1 - d)        formed in float64
    d = decay, or with warm-up min(decay, (1 + k) / (10 + k)), k the averaging updates applied before this one
"""
import numpy as np


def ema_decay_at(decay, k, warmup):
    """The decay the update with ``k`` earlier updates uses, as a float64."""
    d = np.float64(decay)
    if warmup:
        k = np.float64(k)
        d = min(d, (np.float64(1.0) + k) / (np.float64(10.0) + k))
    return d


def ema_weight(decay, k=0, warmup=False):
    return np.float32(np.float64(1.0) - ema_decay_at(decay, k, warmup))


def ema_update(e, p, decay, k=0, warmup=False):
    """One update of the float32 array ``e`` towards ``p``; returns the new array."""
    e, p = np.asarray(e, np.float32), np.asarray(p, np.float32)
    w = ema_weight(decay, k, warmup)
    d = (p - e).astype(np.float32)
    t = (w * d).astype(np.float32)
    return (e + t).astype(np.float32)


def ema_sequence(e0, snapshots, decay, warmup=False, k0=0):
    """``e0`` after one update per snapshot, in order, the count of earlier updates starting at ``k0``."""
    e = np.asarray(e0, np.float32)
    for j, p in enumerate(snapshots):
        e = ema_update(e, p, decay, k0 + j, warmup)
    return e
