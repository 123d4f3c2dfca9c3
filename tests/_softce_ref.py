"""float64 restatements of the soft-target ops — ``avid_soft_ce_loss`` (softmax cross-entropy against a distribution: loss,
gradient, clip-mean confidence, hits) — the float32 error bounds the HIP kernel is held to, the op-by-op float32 restatement
of ``avid_batch_mix`` (mixup, CutMix and the mixed targets: that op is held to torch's float32 expression BIT FOR BIT, so its
restatement is float32 with every operation rounded on its own), and the inputs tests/test_softce_host.py (CPU) and
tests/test_gpu_softce.py (GPU) share.  numpy on the CPU; nothing here is shared with the code under test.

The bounds follow tests/_mlabel_ref.py: c * u * S with u = 2^-24, S the absolute value of the terms an element adds up (from
the float64 reference) and c the roundings on the longest path through csrc/classify.hip: soft_ce_loss_kernel, counted next to
each bound.  expf / logf are budgeted at 1 ulp = 2 u (the device library's documented accuracy), a float32 division at 3 u.
TINY = 2^-126 on top of every per-element bound (a result below the smallest normal float may be flushed to zero).

What every bound shares, per row (d_c = x_c - max, p = softmax, D1 = sum_c p_c |d_c|):
  d_c            one rounding, u |d_c|: a RELATIVE error of u |d_c| in exp(d_c)
  e_c = expf     (2 + |d_c|) u relative
  den = sum e    a thread adds up to 4 columns, the wave butterfly 6 levels, the 4 waves 3 more: 13 additions of positive
                 terms, 13 u, on top of the terms' own weighted mean (2 + D1) u               -> DEN = (15 + D1) u relative
  t'_c           keep = 1 - eps (1), spread = eps / C (3), fmaf (1)                           -> 5 u relative
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126

# (V, clips, C) of the GPU test: one class; a column tail past 64 and past 256; the largest C; more videos than the grid
LOSS_SHAPES = ((1, 1, 1), (3, 2, 10), (5, 1, 65), (4, 3, 101), (2, 2, 1024), (70, 1, 257), (1100, 1, 5))
TARGET_KINDS = ("hard", "two_hot", "unnorm")
SPECIAL_LOGITS = (0.0, -0.0, 30.0, -30.0, 88.8, -88.8)
# (B, Cin, T, H, W) of the mix: plain; rows off 16 bytes; a spectrogram; one pixel
MIX_SHAPES = ((5, 3, 4, 18, 22), (5, 3, 2, 17, 23), (4, 1, 1, 20, 33), (1, 3, 1, 1, 1))
LONG_LAM = float(np.float32(0.3141592741012573))           # a lam with a long mantissa


def _f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def loss_inputs(V, clips, C, kind="hard", seed=0):
    """(logits float32 [V * clips, C], targets float32 [V, C]).  The special logits lead the flattened tensor (as many as fit).
    ``hard``: one-hot rows; ``two_hot``: lam at one class and 1 - lam at another (mixup's targets; C = 1: one-hot);
    ``unnorm``: two-hot rows scaled so that they sum to 0.7 (even videos) and 1.3 (odd videos)."""
    rng = np.random.default_rng(1000 * V + 10 * clips + C + 7919 * seed)
    x = (3.0 * rng.standard_normal((V * clips, C))).astype(np.float32)
    flat = x.reshape(-1)
    k = min(flat.size, len(SPECIAL_LOGITS))
    flat[:k] = np.asarray(SPECIAL_LOGITS[:k], dtype=np.float32)
    t = np.zeros((V, C), np.float32)
    a = rng.integers(C, size=V)
    b = (a + 1 + rng.integers(max(C - 1, 1), size=V)) % C
    lam = rng.uniform(0.55, 0.95, size=V).astype(np.float32)
    for v in range(V):
        if kind == "hard" or C == 1:
            t[v, a[v]] = 1.0
        else:
            t[v, a[v]] = lam[v]
            t[v, b[v]] = np.float32(1.0) - lam[v]
        if kind == "unnorm":
            t[v] *= np.float32(0.7 if v % 2 == 0 else 1.3)
    return x, t


def mix_inputs(shape, seed=0):
    """x float32 of ``shape`` with values whose products with a long-mantissa lam are inexact, signed zeros and a denormal."""
    rng = np.random.default_rng(int(np.prod(shape)) + 7919 * seed)
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    sp = np.asarray([0.0, -0.0, 1e-40, 3.0e38], np.float32)
    flat[:min(flat.size, sp.size)] = sp[:min(flat.size, sp.size)]
    return x


def perms(B):
    """identity, one with a fixed point (sample 0 keeps itself, the rest rotate), a single cycle."""
    ident = np.arange(B, dtype=np.int64)
    fixed = ident.copy()
    if B > 2:
        fixed[1:] = np.roll(ident[1:], 1)
    return {"identity": ident, "fixed_point": fixed, "cycle": np.roll(ident, -1)}


def boxes(H, W):
    """(h0, h1, w0, w1), half-open: empty, the whole plane, one pixel, touching each edge, odd starts."""
    c = lambda v, n: int(min(max(v, 0), n))   # noqa: E731
    return {"empty": (2 % (H + 1), 2 % (H + 1), 0, W), "empty_w": (0, H, c(3, W), c(3, W)), "whole": (0, H, 0, W),
            "pixel": (H // 2, H // 2 + 1, W // 2, W // 2 + 1), "top": (0, c(3, H), c(1, W), c(6, W)),
            "bottom": (c(H - 3, H), H, c(2, W), c(9, W)), "left": (c(1, H), c(5, H), 0, c(5, W)),
            "right": (c(2, H), c(7, H), c(W - 5, W), W), "odd": (c(3, H), c(8, H), c(5, W), c(18, W))}


# ---- the loss ------------------------------------------------------------------------------------------------------------------
def _terms(x, t, clips, eps):
    x, t = _f64(x), _f64(t)
    V, C = t.shape
    x3 = x.reshape(V, clips, C)
    tp = (t * (1.0 - eps) + eps / C)[:, None, :]
    m = x3.max(2, keepdims=True)
    d = x3 - m
    e = np.exp(d)
    den = e.sum(2, keepdims=True)
    lse = np.log(den) + m
    p = e / den
    D1 = (p * np.abs(d)).sum(2, keepdims=True)
    return x3, tp, d, den, lse, p, D1


def loss(x, t, clips=1, eps=0.0):
    """mean over the V * clips rows of sum_c t'_c (lse - x_c), t' = t (1 - eps) + eps / C."""
    x3, tp, _, _, lse, _, _ = _terms(x, t, clips, eps)
    return float((tp * (lse - x3)).sum(2).mean())


def loss_bound(x, t, clips=1, eps=0.0):
    """lse = logf(den) + m: DEN absolute, logf 2 u |log den|, the sum u |lse|.  A term t'_c (lse - x_c): the difference u |lse -
    x_c| on top of lse's error, t' 5 u, the product 1: t'_c (7 u |lse - x_c| + E), E = (15 + D1 + 2 |log den| + |lse|) u.  The
    terms are added in double (dropped); the mean is rounded to float once: u |loss|."""
    x3, tp, _, den, lse, _, D1 = _terms(x, t, clips, eps)
    E = (15.0 + D1 + 2.0 * np.abs(np.log(den)) + np.abs(lse)) * U
    row = (np.abs(tp) * (7.0 * U * np.abs(lse - x3) + E)).sum(2)
    return float(row.mean()) + U * abs(loss(x, t, clips, eps)) + TINY


def grad(x, t, clips=1, eps=0.0, grad_scale=1.0):
    """d(loss * grad_scale) / d logits = (p_c S - t'_c) * grad_scale / (V clips), S = sum_c t'_c: [V * clips, C]."""
    x3, tp, _, _, _, p, _ = _terms(x, t, clips, eps)
    S = tp.sum(2, keepdims=True)
    return ((p * S - tp) * (grad_scale / (x3.shape[0] * x3.shape[1]))).reshape(-1, x3.shape[2])


def grad_bound(x, t, clips=1, eps=0.0, grad_scale=1.0):
    """p_c = e_c / den: (2 + |d_c|) + DEN + the division 3 + the product 1 = (21 + |d_c| + D1) u.  S: the terms' 5 u and 13
    additions, 18 u.  p S: 1 more -> (40 + |d_c| + D1) u.  The difference: 1 on |p S| and on |t'| (5 u of its own).  The scale
    grad_scale / rows (conversion 1, division 3) and the product with it 1: 5 on both.
    -> (46 + |d_c| + D1) u p S + 11 u t', times the scale."""
    x3, tp, d, _, _, p, D1 = _terms(x, t, clips, eps)
    S = np.abs(tp).sum(2, keepdims=True)
    sc = abs(grad_scale) / (x3.shape[0] * x3.shape[1])
    return ((((46.0 + np.abs(d) + D1) * p * S + 11.0 * np.abs(tp)) * U + TINY) * sc).reshape(-1, x3.shape[2])


def confidence(x, t, clips=1):
    """[V, C]: the mean over a video's clips of softmax(row)."""
    _, _, _, _, _, p, _ = _terms(x, t, clips, 0.0)
    return p.mean(1)


def confidence_bound(x, t, clips=1):
    """p_c (21 + |d_c| + D1) u per clip; clips - 1 additions of positive terms, 1 / clips (3) and the product with it (1):
    (clips + 3) u conf."""
    _, _, d, _, _, p, D1 = _terms(x, t, clips, 0.0)
    return ((21.0 + np.abs(d) + D1) * p).mean(1) * U + (clips + 3) * U * p.mean(1) + TINY


def hits(conf, t):
    """(top-1 hits, top-5 hits) by ``avid_cls_loss``'s rank rule: a video's label is the argmax of its target row (numpy: the
    first maximum, the lower index); its rank is the number of classes with a strictly higher confidence, or an equal one at
    a lower index; a hit is rank < 1 / rank < 5."""
    conf, t = np.asarray(conf), _f64(t)
    lab = np.argmax(t, axis=1)
    cl = conf[np.arange(conf.shape[0]), lab][:, None]
    idx = np.arange(conf.shape[1])[None, :]
    above = ((conf > cl) | ((conf == cl) & (idx < lab[:, None]))).sum(1)
    return int((above < 1).sum()), int((above < 5).sum())


# ---- the mix, float32 operation by operation ----------------------------------------------------------------------------------------
def _bcast(lam, ndim):
    return np.asarray(lam, np.float32).reshape((-1,) + (1,) * (ndim - 1))


def mixup(x, perm, lam):
    """y = lam * x + (1 - lam) * x[perm]: two float32 products, one difference, one sum, each rounded on its own (numpy rounds
    every float32 operation; it never contracts)."""
    x = np.asarray(x, np.float32)
    l = _bcast(lam, x.ndim)
    a = (l * x).astype(np.float32)
    b = ((np.float32(1.0) - l).astype(np.float32) * x[np.asarray(perm)]).astype(np.float32)
    return (a + b).astype(np.float32)


def mixup_fma(x, perm, lam):
    """The defect the bit-for-bit tests have to see: lam * x + ((1 - lam) * x[perm]) with the first product and the sum
    contracted into one fma (computed in double and rounded once: exact for float32 operands)."""
    x = np.asarray(x, np.float32)
    l = _bcast(lam, x.ndim)
    b = ((np.float32(1.0) - l).astype(np.float32) * x[np.asarray(perm)]).astype(np.float32)
    with np.errstate(over="ignore"):
        return (l.astype(np.float64) * x.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def cutmix(x, perm, box):
    """y[b][..., h0:h1, w0:w1] = x[perm[b]][..., h0:h1, w0:w1], x[b] elsewhere: slicing."""
    x = np.asarray(x, np.float32)
    y = x.copy()
    for b, (h0, h1, w0, w1) in enumerate(np.asarray(box)):
        y[b, ..., h0:h1, w0:w1] = x[perm[b], ..., h0:h1, w0:w1]
    return y


def one_hot(labels, C):
    t = np.zeros((len(labels), C), np.float32)
    for b, l in enumerate(labels):
        if 0 <= l < C:
            t[b, l] = 1.0
    return t


def mix_targets(t, perm, lam):
    """t_out = lam * t + (1 - lam) * t[perm] by the same four roundings; ``t`` float32 [B, C]."""
    return mixup(t, perm, lam)
