"""float64 restatements of the multi-label ops — ``avid_mlabel_loss`` (binary cross-entropy with logits: loss, gradient,
clip-mean confidence, hits) and ``avid_rank_metrics`` (per-class average precision and ROC-AUC in their counting forms) — the
float32 error bounds the HIP kernels are held to, and the inputs tests/test_mlabel_host.py (CPU) and tests/test_gpu_mlabel.py
(GPU) share.  numpy on the CPU; nothing here is shared with the code under test.

The loss bounds follow tests/_width_ref.py: c * u * S with u = 2^-24, S the sum of the absolute values of the terms an element
adds up (from the float64 reference) and c the roundings on the longest path through csrc/classify.hip: mlabel_loss_kernel,
counted next to each bound.  expf / log1pf are budgeted at 1 ulp = 2 u (the device library's documented accuracy), a float32
division at 3 u.  TINY = 2^-126 on top of every per-element bound: a result below the smallest normal float (exp(-88.8) is
one) has no relative accuracy and may be flushed to zero.

The metrics have no float32 arithmetic: counts are integers, the precisions and the two divisions are double.  Their tolerance
is the summation's: (2 P + 8) * 2^-53 for AP (one double rounding per term and per addition on either side, terms <= 1), one
rounding for AUC.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
D = 2.0 ** -53

# (V, clips, C): one element; under / exactly / past one 64-lane wave; several clips; AudioSet's class count over three of the
# kernel's four column slots; more videos than one workgroup per 256 and the widest row
LOSS_SHAPES = ((1, 1, 1), (2, 1, 63), (3, 2, 64), (7, 3, 65), (5, 10, 527), (257, 1, 1024))
SPECIAL_LOGITS = (0.0, -0.0, 30.0, -30.0, 88.8, -88.8, 104.0, -104.0)
RANK_N = (1, 2, 63, 64, 65, 1000, 4099)
RANK_C = (1, 3, 64, 65, 527)


def _f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def loss_inputs(V, clips, C, soft=False, with_pw=False, seed=0):
    """(logits float32 [V * clips, C], targets float32 [V, C], pos_weight float32 [C] or None).  The special logits lead the
    flattened tensor (as many as fit); targets are {0, 1}, or with ``soft`` drawn from {0, 0.25, 0.5, 1}."""
    rng = np.random.default_rng(1000 * V + 10 * clips + C + 7919 * seed)
    x = (3.0 * rng.standard_normal((V * clips, C))).astype(np.float32)
    flat = x.reshape(-1)
    k = min(flat.size, len(SPECIAL_LOGITS))
    flat[:k] = np.asarray(SPECIAL_LOGITS[:k], dtype=np.float32)
    t = rng.choice(np.asarray([0.0, 0.25, 0.5, 1.0]) if soft else np.asarray([0.0, 1.0]), size=(V, C),
                   p=(0.4, 0.2, 0.2, 0.2) if soft else (0.8, 0.2)).astype(np.float32)
    pw = rng.uniform(0.5, 20.0, size=C).astype(np.float32) if with_pw else None
    return x, t, pw


def rank_inputs(N, C, seed=0):
    """(scores float32 [N, C], targets float32 [N, C]) with the columns the issue names, as far as C holds them: scores rounded
    to one decimal everywhere (ties); column 0 of mixed +-0.0; column 1 all equal; column 2 without positives; column 3 all
    positive; column 4 with one NaN score; the last column (C >= 6) holds +-inf."""
    rng = np.random.default_rng(100003 * N + C + 7919 * seed)
    s = np.round(rng.standard_normal((N, C)), 1).astype(np.float32)
    t = (rng.random((N, C)) < 0.3).astype(np.float32)
    s[:, 0] = np.where(rng.random(N) < 0.5, np.float32(0.0), np.float32(-0.0))
    if C > 1:
        s[:, 1] = np.float32(0.7)
    if C > 2:
        t[:, 2] = 0.0
    if C > 3:
        t[:, 3] = 1.0
    if C > 4:
        s[N // 2, 4] = np.nan
    if C > 5:
        s[::3, C - 1] = np.inf
        s[1::3, C - 1] = -np.inf
    return s, t


# ---- the loss ------------------------------------------------------------------------------------------------------------------
def _terms(x, t, pw, clips):
    x, t = _f64(x), _f64(t)
    V, C = t.shape
    x3 = x.reshape(V, clips, C)
    t3 = t[:, None, :]
    pwv = np.ones(C) if pw is None else _f64(pw)
    w = 1.0 + (pwv - 1.0)[None, None, :] * t3
    wabs = 1.0 + np.abs(pwv - 1.0)[None, None, :] * t3           # the terms w adds up, in absolute value
    sp = np.log1p(np.exp(-np.abs(x3))) + np.maximum(-x3, 0.0)    # softplus(-x), stable
    e = np.exp(-np.abs(x3))
    sig = np.where(x3 >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    q = np.where(x3 >= 0, e / (1.0 + e), 1.0 / (1.0 + e))        # 1 - sigmoid(x) without the cancellation
    return x3, t3, w, wabs, sp, sig, q


def loss(x, t, pw=None, clips=1):
    """mean over all V * clips * C elements of (1 - t) x + w softplus(-x), w = 1 + (pw - 1) t."""
    x3, t3, w, _, sp, _, _ = _terms(x, t, pw, clips)
    return float(((1.0 - t3) * x3 + w * sp).mean())


def loss_bound(x, t, pw=None, clips=1):
    """Per element: e = expf(-|x|) 2 u; log1pf(e) its argument's 2 u (d log1p / d e * e <= log1p(e)) + its own 2 u, + the sum with
    max(-x, 0): softplus 5 u.  a = 1 - t: 1.  w = 1 + (pw - 1) t: 3 roundings on |1| + |pw - 1| t = wabs.  a x: 2 u |a x|;
    w softplus: (5 + 3 + 1) u wabs softplus; the sum of the two: 1 more on both.  -> 10 u S, S = |a x| + wabs softplus.  The
    elements are added in double (n 2^-53: dropped) and the mean is rounded to float once: 11 u mean(S)."""
    x3, t3, _, wabs, sp, _, _ = _terms(x, t, pw, clips)
    S = np.abs((1.0 - t3) * x3) + wabs * sp
    return 11 * U * float(S.mean()) + TINY * float(wabs.mean())


def grad(x, t, pw=None, clips=1, grad_scale=1.0):
    """d(loss * grad_scale) / d logits = ((1 - t) - w (1 - sigmoid(x))) * grad_scale / (V clips C), [V * clips, C]."""
    x3, t3, w, _, _, _, q = _terms(x, t, pw, clips)
    return (((1.0 - t3) - w * q) * (grad_scale / x3.size)).reshape(-1, x3.shape[2])


def grad_bound(x, t, pw=None, clips=1, grad_scale=1.0):
    """q = 1 - sigmoid(x) is e r or r, r = 1 / (1 + e): e 2 u, the sum 1, the division 3, the product with e 2 + 1: 9 u.
    w q: (3 + 9 + 1) u wabs q; a: 1; the subtraction 1 on both; the scale grad_scale / n (conversion 1, division 3) and the
    product with it 1: 5 on both -> 7 u |a| + 19 u wabs q <= 20 u S, S = (|a| + wabs q) * scale."""
    x3, t3, _, wabs, _, _, q = _terms(x, t, pw, clips)
    sc = abs(grad_scale) / x3.size
    return ((20 * U * (np.abs(1.0 - t3) + wabs * q) + TINY * wabs) * sc).reshape(-1, x3.shape[2])


def confidence(x, t, clips=1):
    """[V, C]: the mean over a video's clips of sigmoid(x)."""
    _, _, _, _, _, sig, _ = _terms(x, t, None, clips)
    return sig.mean(1)


def confidence_bound(x, t, clips=1):
    """sigmoid 9 u (as q above), clips - 1 additions of positive terms, one division by clips (3): (clips + 11) u conf."""
    return (clips + 11) * U * confidence(x, t, clips) + TINY


def hits(conf, t):
    """(videos whose highest-confidence class — ties to the lower index — is positive, (video, class) pairs with
    (conf >= 0.5) == (t >= 0.5)); a class is positive iff t >= 0.5."""
    conf, t = np.asarray(conf), _f64(t)
    top = np.argmax(conf, axis=1)                        # (numpy: the first maximum)
    return int((t[np.arange(t.shape[0]), top] >= 0.5).sum()), int(((conf >= 0.5) == (t >= 0.5)).sum())


# ---- the metrics ---------------------------------------------------------------------------------------------------------------
def _counts(s, pos):
    """Per positive, in ascending sample index: (#pos >= s_i, #neg >= s_i, #neg > s_i), by binary search in the sorted
    positives / negatives — the counting definitions, not a ranking of the samples."""
    sp, sn = np.sort(s[pos]), np.sort(s[~pos])
    si = s[pos]
    tp = sp.size - np.searchsorted(sp, si, side="left")
    fp_ge = sn.size - np.searchsorted(sn, si, side="left")
    fp_gt = sn.size - np.searchsorted(sn, si, side="right")
    return tp, fp_ge, fp_gt


def rank_metrics(scores, targets):
    """(ap float64 [C], auc float64 [C], n_pos int64 [C]).  ap_c = (1 / P) sum over positives, in ascending sample index and in
    double, of TP_i / (TP_i + FP_i); auc_c = U2 / (2 P Nn) with U2 = sum of 2 #{neg < s_i} + #{neg == s_i} an integer.  NaN
    where undefined (P = 0; for auc also Nn = 0) and for a class with a NaN score."""
    s_all = np.asarray(scores, dtype=np.float32)
    t_all = _f64(targets)
    N, C = s_all.shape
    ap, auc, n_pos = np.full(C, np.nan), np.full(C, np.nan), np.zeros(C, dtype=np.int64)
    for c in range(C):
        s, pos = s_all[:, c], t_all[:, c] >= 0.5
        P = int(pos.sum())
        Nn = N - P
        n_pos[c] = P
        if P == 0 or np.isnan(s).any():
            continue
        tp, fp_ge, fp_gt = _counts(s, pos)
        terms = tp.astype(np.float64) / (tp + fp_ge).astype(np.float64)
        ap[c] = np.cumsum(terms)[-1] / P                  # (cumsum adds one term after the other)
        if Nn:
            u2 = int((2 * (Nn - fp_ge) + (fp_ge - fp_gt)).astype(np.int64).sum())
            auc[c] = u2 / (2 * P * Nn)
    return ap, auc, n_pos


def ap_tolerance(n_pos):
    return (2.0 * np.asarray(n_pos, dtype=np.float64) + 8.0) * D


def d_prime(mauc):
    from scipy.special import ndtri
    return math.sqrt(2.0) * float(ndtri(mauc))
