"""The step guard restated for the tests (include/avid_hip.h: ``avid_grad_guard`` and the guarded optimizers).

``guard_ref``: norm, coefficient and skip word in float64 from the exactly rounded sum of the exact squares — the yardstick.
``kernel_norm``: the kernel's own summation, same partition, same order, same number formats (fp32 gradients, products
and partial sums in double, one rounding to fp32 at the end), in numpy — what the error bound is derived from.
``norm_bound``: that bound.  ``adam_clipped`` / ``sgd_clipped``: float64 / float32 optimizer steps on
``(g * grad_scale) * clip_coef``."""
import math

import numpy as np

from _sgd_ref import sgd_step

THREADS, MAX_BLOCKS = 256, 1024          # csrc/optim.hip: GUARD_THREADS, GUARD_MAX_BLOCKS
GRID_STRIDE = MAX_BLOCKS * THREADS * 4   # floats one full grid of 16-byte loads covers
FLT_MAX = float(np.finfo(np.float32).max)
EPS_CLIP = float(np.float32(1e-6))       # the kernel's 1e-6f


def blocks_of(n):
    return min(MAX_BLOCKS, max(1, -(-n // (THREADS * 4))))


def partition(n, start):
    """(head, n4, tail) of a slice of n floats that begins ``start`` floats behind a 16-byte boundary."""
    head = min((4 - start % 4) % 4, n)
    n4 = (n - head) // 4
    return head, n4, n - head - 4 * n4


def _block_sum(s):
    """[blocks, 256] doubles -> [blocks]: the xor butterfly over each 64-lane wave, then the four waves left to right."""
    s = s.reshape(-1, 4, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    w = s[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def kernel_sum(g, start=0, drop_tail=False, drop_slice=False):
    """The kernel's double sum of squares of the fp32 array ``g``.  ``drop_tail`` / ``drop_slice``: the same with a bug — the
    last scalar tail element, or 64 floats in the middle of the vector body, left out."""
    g = np.asarray(g, np.float32)
    n = g.size
    head, n4, tail = partition(n, start)
    blocks = blocks_of(n)
    T = blocks * THREADS
    body = g[head:head + 4 * n4].astype(np.float64).reshape(n4, 4)
    sq = body * body                                   # exact: 24-bit x 24-bit significands
    if drop_slice:
        assert n4 >= 32
        sq[n4 // 2 - 8:n4 // 2 + 8] = 0.0
    L = -(-n4 // T) if n4 else 0
    pad = np.zeros((L * T, 4))
    pad[:n4] = sq
    acc = np.zeros((T, 4))
    for it in pad.reshape(L, T, 4):                    # round `it` of the grid-stride loop (x + 0.0 == x: the padding is inert)
        acc = acc + it
    for t in range(head):                              # block 0, threads 0 .. head-1: the scalar head
        acc[t, 0] += float(g[t]) * float(g[t])
    for k in range(tail - (1 if drop_tail else 0)):    # ... the threads behind them: the scalar tail
        x = float(g[head + 4 * n4 + k])
        acc[head + k, 0] += x * x
    parts = _block_sum((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3]))
    P = -(-blocks // THREADS)
    pp = np.zeros(P * THREADS)
    pp[:blocks] = parts
    a = np.zeros(THREADS)
    for row in pp.reshape(P, THREADS):                 # thread t: partials t, t + 256, ... in that order
        a = a + row
    return float(_block_sum(a[None, :])[0])


def kernel_norm(g, grad_scale, start=0, scale_twice=False, **bug):
    """``grad_norm`` as the kernel forms it (fp32).  ``scale_twice``: the bug of applying ``grad_scale`` twice."""
    s = kernel_sum(g, start, **bug)
    norm = math.sqrt(s) * float(np.float32(grad_scale))
    if scale_twice:
        norm *= float(np.float32(grad_scale))
    return float(np.float32(norm))


def chain_length(n):
    """The most additions any one square goes through on its way into the sum: the grid-stride rounds of a thread, the
    scalar element, (a0 + a1) + (a2 + a3), six butterfly levels, three wave additions; then the partials of a thread of the
    finishing block, six levels, three additions."""
    blocks = blocks_of(n)
    rounds = -(-(n // 4) // (blocks * THREADS))
    return rounds + 1 + 2 + 6 + 3 + -(-blocks // THREADS) + 6 + 3


def norm_bound(n):
    """Relative error bound of ``grad_norm``.  All terms are >= 0 and the squares are exact in double, so
    the sum is within k u64 / (1 - k u64) of exact (k = ``chain_length``, u64 = 2^-53); the square root halves that and adds
    u64, the product with ``grad_scale`` adds u64, the one rounding to fp32 adds u32 = 2^-24 — (k / 2 + 3) u64 covers the
    double part with its second-order terms.  A result below the fp32 normal range carries 2^-150 absolute instead."""
    return 2.0 ** -24 + (chain_length(n) / 2 + 3) * 2.0 ** -53


def guard_ref(g, grad_scale=1.0, max_norm=0.0, skip_nonfinite=True):
    """float64: {"norm", "coef", "skip", "finite"} for the fp32 array ``g`` (``grad_scale`` / ``max_norm`` as the fp32 values
    the C ABI carries).  The sum is judged as fp32: above FLT_MAX it is an overflow and the norm is inf."""
    g64 = np.asarray(g, np.float32).astype(np.float64)
    scale, max_norm = float(np.float32(grad_scale)), float(np.float32(max_norm))
    with np.errstate(over="ignore", invalid="ignore"):
        sq = g64 * g64
        finite = bool(np.isfinite(sq).all())
        if not finite:
            s = float(np.sum(sq))
        elif sq.size <= 1 << 20:
            s = math.fsum(sq.tolist())                 # the exactly rounded sum of the exact squares
        else:                                          # (a list of 21 M Python floats is too much: pairwise in 64-bit significands)
            s = float(np.sum(sq.astype(np.longdouble)))
    finite = finite and s <= FLT_MAX * (1 + 2.0 ** -25)
    norm = math.sqrt(s) * scale if finite else (float("nan") if math.isnan(s) else float("inf"))
    coef = 1.0
    if max_norm > 0 and not math.isnan(norm):
        coef = min(1.0, max_norm / (norm + EPS_CLIP))
    skip = bool(skip_nonfinite) and not finite
    return {"norm": norm, "coef": 1.0 if skip else coef, "skip": int(skip), "finite": finite}


def adam_clipped(p, g, m, v, lr, b1, b2, eps, wd, t, grad_scale, coef):
    """One float64 torch.optim.Adam step (L2 weight decay in the gradient, bias-corrected) on (g * grad_scale) * coef, with the
    hyper-parameters as the fp32 values the C ABI carries.  Returns (p, m, v)."""
    lr, b1, b2, eps, wd, grad_scale = (float(np.float32(x)) for x in (lr, b1, b2, eps, wd, grad_scale))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gg = g * grad_scale * float(coef) + wd * p
    m = b1 * m + (1 - b1) * gg
    v = b2 * v + (1 - b2) * gg * gg
    denom = np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps
    return p - lr / (1 - b1 ** t) * (m / denom), m, v


def sgd_clipped(p, g, buf, lr, momentum, wd, nesterov, grad_scale, coef, dtype=np.float32):
    """torch's single-tensor SGD (tests/_sgd_ref.py) on (g * grad_scale) * coef, the two products rounded one after the
    other in ``dtype``: the bit reference of ``avid_sgd_flat_guarded`` in float32."""
    T = np.dtype(dtype).type
    d = np.asarray(g, dtype) * T(grad_scale)
    return sgd_step(np.asarray(p, dtype), d, buf, lr, momentum, wd, nesterov, T(coef), dtype)
