"""The table-driven optimizers restated in numpy, one operation per statement (the style of tests/_sgd_ref.py): grouped SGD, grouped
Adam, LARS and LAMB over a flat buffer whose tensors ("segments") take their own ``lr_scale`` / ``weight_decay`` / ``adapt``.

A table is a list of ``Seg(offset, numel, lr_scale, weight_decay, adapt)``; the arrays are the whole flat buffers, padding between
the segments included, and what a function returns differs from what it was given only inside the segments.

Run in float32 — arrays and hyper-parameters alike, every product and every sum rounded on its own — the SGD family (grouped SGD,
LARS) is the BIT reference of ``avid_sgd_flat_table``; the Adam family is the kernels' arithmetic up to their two fused
multiply-adds (numpy has none: they are formed in float64 and rounded once more, which differs from the fused result by a
double rounding in about one element in 2^29).  Run in float64 every function is the yardstick: float64 arithmetic ON THE
FLOAT32 VALUES of the hyper-parameters (the C ABI takes them as ``float``), so that what is left is the arithmetic alone.

Segment norms come from ``math.fsum`` of the squares: of float32 values these are exact in float64, so the sum is the correctly
rounded exact sum — what the kernels' double accumulation in a fixed order is held against."""
import math
from collections import namedtuple

import numpy as np

Seg = namedtuple("Seg", "offset numel lr_scale weight_decay adapt")
U = 2.0 ** -24                                  # unit roundoff of float32


def padded_table(numels, lr_scale=1.0, weight_decay=0.0, adapt=True):
    """Segments of the given lengths laid out as ``parallel.FlatParams`` lays tensors out: each starts on a multiple of 4 floats.
    ``lr_scale`` / ``weight_decay`` / ``adapt``: one value, or one per segment.  Returns (segments, elements of the buffer)."""
    def each(v):
        return list(v) if isinstance(v, (list, tuple)) else [v] * len(numels)
    segs, off = [], 0
    for n, s, w, a in zip(numels, each(lr_scale), each(weight_decay), each(adapt)):
        segs.append(Seg(off, int(n), float(s), float(w), bool(a)))
        off += (int(n) + 3) // 4 * 4
    return segs, off


def padding_mask(segs, n):
    """True on the elements of no segment."""
    m = np.ones(n, bool)
    for s in segs:
        m[s.offset:s.offset + s.numel] = False
    return m


def f32(x):
    """The float32 value of a hyper-parameter as a Python float (what the C ABI sees)."""
    return float(np.float32(x))


def sumsq(x):
    """The sum of the squares of ``x`` as a Python float: for float32 input the correctly rounded exact sum (the products are exact in
    float64, ``fsum`` adds them without error)."""
    x = np.asarray(x)
    if x.dtype == np.float64:          # the yardstick's own norms: products round anyway, a long-double sum is ample
        return float(np.sum(x * x, dtype=np.longdouble))
    x = x.astype(np.float64)
    return math.fsum(x * x)


def segment_sumsq(x, segs):
    return [sumsq(x[s.offset:s.offset + s.numel]) for s in segs]


def _sgd_d(p, g, wd, grad_scale, coef):
    d = g * grad_scale
    d = d * coef
    if wd != 0:
        t = wd * p
        d = d + t
    return d


def lars_q(p, g, segs, trust_coefficient, grad_scale=1.0, coef=1.0, dtype=np.float32):
    """Per segment ``q = trust_coefficient * |p| / |d|`` with ``d = (g * grad_scale) * coef + wd * p`` computed in ``dtype`` and the
    norms from ``fsum``: formed in double, rounded once to ``dtype``; 1 for a segment that is not adapted or has a zero norm."""
    T = np.dtype(dtype).type
    out = []
    for s in segs:
        sl = slice(s.offset, s.offset + s.numel)
        d = _sgd_d(p[sl], g[sl], T(f32(s.weight_decay)), T(f32(grad_scale)), T(f32(coef)))
        sp, sd = sumsq(p[sl]), sumsq(d)
        q = 1.0
        if s.adapt and sp > 0.0 and sd > 0.0:
            q = f32(trust_coefficient) * (math.sqrt(sp) / math.sqrt(sd))
        out.append(T(q))
    return out


def grouped_sgd_step(p, g, buf, segs, lr, momentum, nesterov=False, grad_scale=1.0, coef=1.0, q=None, dtype=np.float32):
    """One step of grouped SGD; ``q`` (one factor per segment, e.g. ``lars_q``'s) makes it LARS: the factor multiplies ``d`` behind the
    weight-decay term and in front of the momentum.  ``buf`` is None exactly when ``momentum == 0``.  Returns the new (p, buf)."""
    T = np.dtype(dtype).type
    assert p.dtype == g.dtype == np.dtype(dtype) and (buf is None) == (momentum == 0) and not (nesterov and momentum == 0)
    lr, momentum, grad_scale, coef = T(f32(lr)), T(f32(momentum)), T(f32(grad_scale)), T(f32(coef))
    p, buf = p.copy(), (None if buf is None else buf.copy())
    for k, s in enumerate(segs):
        sl = slice(s.offset, s.offset + s.numel)
        lr_s = lr * T(f32(s.lr_scale))
        d = _sgd_d(p[sl], g[sl], T(f32(s.weight_decay)), grad_scale, coef)
        if q is not None:
            d = T(q[k]) * d
        if momentum != 0:
            t = momentum * buf[sl]
            b = t + d
            buf[sl] = b
            if nesterov:
                t = momentum * b
                d = d + t
            else:
                d = b
        t = lr_s * d
        p[sl] = p[sl] - t
    return p, buf


def lars_step(p, g, buf, segs, lr, momentum, nesterov, trust_coefficient, grad_scale=1.0, coef=1.0, dtype=np.float32):
    """(p, buf, q): ``lars_q`` then ``grouped_sgd_step`` with it."""
    q = lars_q(p, g, segs, trust_coefficient, grad_scale, coef, dtype)
    p, buf = grouped_sgd_step(p, g, buf, segs, lr, momentum, nesterov, grad_scale, coef, q, dtype)
    return p, buf, q


def _fma(a, b, c, dtype):
    """a * b + c with one rounding in float64 and, for float32, one more to float32."""
    if np.dtype(dtype) == np.float64:
        return a * b + c
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _bias_corrections(beta1, beta2, step):
    bc1 = 1.0 - f32(beta1) ** step
    bc2 = 1.0 - f32(beta2) ** step
    return bc1, bc2


def grouped_adam_step(p, g, m, v, segs, lr, beta1, beta2, eps, step, grad_scale=1.0, dtype=np.float32):
    """torch.optim.Adam's update (L2 decay folded into the gradient) with per-segment lr and decay, the kernel's operations:
    gg = g * grad_scale + wd * p; m = b1 m + (1 - b1) gg; v = b2 v + ((1 - b2) gg) gg; p -= step_size * (m / (sqrt(v) * c2 + eps)),
    step_size = lr_s / (1 - b1^t) rounded once, c2 = 1 / sqrt(1 - b2^t) rounded once.  Returns the new (p, m, v)."""
    T = np.dtype(dtype).type
    b1, b2, eps_, gs = T(f32(beta1)), T(f32(beta2)), T(f32(eps)), T(f32(grad_scale))
    bc1, bc2 = _bias_corrections(beta1, beta2, step)
    c2 = T(1.0 / math.sqrt(bc2))
    one = T(1)
    p, m, v = p.copy(), m.copy(), v.copy()
    for s in segs:
        sl = slice(s.offset, s.offset + s.numel)
        lr_s = T(f32(lr)) * T(f32(s.lr_scale))
        step_size = T(float(lr_s) / bc1)
        t = T(f32(s.weight_decay)) * p[sl]
        gg = _fma(g[sl], gs, t, dtype)
        a = (one - b1) * gg
        m[sl] = _fma(b1, m[sl], a, dtype)
        d = (one - b2) * gg
        d = d * gg
        v[sl] = _fma(b2, v[sl], d, dtype)
        den = _fma(np.sqrt(v[sl]), c2, eps_, dtype)
        r = m[sl] / den
        p[sl] = _fma(-step_size, r, p[sl], dtype)
    return p, m, v


def lamb_u(p, m, v, wd, c1, c2, eps):
    mh = m * c1
    den = np.sqrt(v) * c2
    den = den + eps
    u = mh / den
    if wd != 0:
        t = wd * p
        u = u + t
    return u


def lamb_step(p, g, m, v, segs, lr, beta1, beta2, eps, step, grad_scale=1.0, coef=1.0, dtype=np.float32, ratios=None,
              norm_extra=None):
    """One LAMB step.  Adam's moments of gt = (g * grad_scale) * coef without an L2 term; u = (m * c1) / (sqrt(v) * c2 + eps) +
    wd * p with c1 = 1 / (1 - b1^t), c2 = 1 / sqrt(1 - b2^t) each rounded once; r = |p| / |u| per adapted segment with two
    norms > 0 (fsum), formed in double and rounded once, else 1; p = p - ((lr * lr_scale) * r) * u.
    ``ratios`` (testing): use these instead of the computed ones.  ``norm_extra`` (testing): per segment a slice whose elements
    are counted into both norms as well.  Returns the new (p, m, v) and the list of ratios."""
    T = np.dtype(dtype).type
    b1, b2, eps_, gs, cf = T(f32(beta1)), T(f32(beta2)), T(f32(eps)), T(f32(grad_scale)), T(f32(coef))
    bc1, bc2 = _bias_corrections(beta1, beta2, step)
    c1, c2 = T(1.0 / bc1), T(1.0 / math.sqrt(bc2))
    one = T(1)
    p, m, v = p.copy(), m.copy(), v.copy()
    used = []
    for k, s in enumerate(segs):
        sl = slice(s.offset, s.offset + s.numel)
        wd = T(f32(s.weight_decay))
        gg = g[sl] * gs
        gg = gg * cf
        a = (one - b1) * gg
        m[sl] = _fma(b1, m[sl], a, dtype)
        d = (one - b2) * gg
        d = d * gg
        v[sl] = _fma(b2, v[sl], d, dtype)
        u = lamb_u(p[sl], m[sl], v[sl], wd, c1, c2, eps_)
        sp, su = sumsq(p[sl]), sumsq(u)
        if norm_extra is not None and norm_extra[k] is not None:
            ex = norm_extra[k]
            sp += sumsq(p[ex])
            su += sumsq(lamb_u(p[ex], m[ex], v[ex], wd, c1, c2, eps_))
        r = 1.0
        if s.adapt and sp > 0.0 and su > 0.0:
            r = math.sqrt(sp) / math.sqrt(su)
        r = T(r) if ratios is None else T(ratios[k])
        used.append(r)
        lr_s = T(f32(lr)) * T(f32(s.lr_scale))
        st = lr_s * r
        t = st * u
        p[sl] = p[sl] - t
    return p, m, v, used


class LambBound:
    """A running, per-element bound on |float32 LAMB - float64 LAMB| for p, m and v, carried from step to step next to the
    float64 yardstick (the way tests/_width_ref.py counts operations).  Every float32 operation contributes U = 2^-24 times
    the magnitude of its result, every earlier error is carried through the operation's derivative; terms of second order
    in U are covered by the factor SECOND.  Per step and element, with ' the float64 values:

      gg = (g gs) coef                      e_gg = 2 U |gg|
      m  = fma(b1, m, (1 - b1) gg)          e_m  = b1 e_m + c e_gg + 2 U |c gg| + U |m|         (1 - b1 itself is rounded)
      v  = fma(b2, v, ((1 - b2) gg) gg)     e_v  = b2 e_v + 2 c |gg| e_gg + 3 U |c gg^2| + U |v|
      mh = m c1                             e_mh = c1 e_m + 2 U |mh|                            (c1 itself is rounded)
      s  = sqrt(v)                          e_s  = min(e_v / sqrt(v), sqrt(e_v)) + U s
      den = s c2 + eps                      e_den = c2 e_s + 2 U |s c2| + U |den|
      r  = mh / den                         e_r  = (e_mh + |r| e_den) / (den - e_den) + U |r|
      u  = r + wd p                         e_u  = e_r + wd e_p + U |wd p| + U |u|
      R  = |p| / |u|  (segment)             e_R  = (|e_p|_2 + R |e_u|_2) / (|u|_2 - |e_u|_2) + 2 U R   (norms in double, one rounding; the
                                                   second U covers the double accumulation many times over)
      st = (lr scale) R                     e_st = lr_s e_R + 2 U st
      p  = p - st u                         e_p  = e_p + st e_u + |u| e_st + U |st u| + U |p|"""
    SECOND = 1.001

    def __init__(self, n):
        self.ep, self.em, self.ev = np.zeros(n), np.zeros(n), np.zeros(n)

    def step(self, p, g, m, v, segs, lr, beta1, beta2, eps, step, grad_scale=1.0, coef=1.0):
        """Advance the yardstick (float64 arrays ``p``, ``m``, ``v``; ``g`` float64) by one step; returns the new (p, m, v) and leaves the
        bounds of the NEW values in ``ep`` / ``em`` / ``ev``."""
        b1, b2, eps_, gs, cf = f32(beta1), f32(beta2), f32(eps), f32(grad_scale), f32(coef)
        bc1, bc2 = _bias_corrections(beta1, beta2, step)
        c1, c2 = 1.0 / bc1, 1.0 / math.sqrt(bc2)
        p2, m2, v2, _ = lamb_step(p, g, m, v, segs, lr, beta1, beta2, eps, step, grad_scale, coef, np.float64)
        ep, em, ev = self.ep.copy(), self.em.copy(), self.ev.copy()
        for s in segs:
            sl = slice(s.offset, s.offset + s.numel)
            wd, lr_s = f32(s.weight_decay), f32(lr) * f32(s.lr_scale)
            gg = np.abs(g[sl] * gs * cf)
            e_gg = 2 * U * gg
            e_m = b1 * em[sl] + (1 - b1) * e_gg + 2 * U * (1 - b1) * gg + U * np.abs(m2[sl])
            e_v = b2 * ev[sl] + 2 * (1 - b2) * gg * e_gg + 3 * U * (1 - b2) * gg * gg + U * np.abs(v2[sl])
            mh = np.abs(m2[sl]) * c1
            e_mh = c1 * e_m + 2 * U * mh
            sq = np.sqrt(v2[sl])
            with np.errstate(divide="ignore", invalid="ignore"):
                e_s = np.minimum(np.where(sq > 0, e_v / sq, np.inf), np.sqrt(e_v)) + U * sq
            den = sq * c2 + eps_
            e_den = c2 * e_s + 2 * U * sq * c2 + U * den
            r = mh / den
            e_r = (e_mh + r * e_den) / np.maximum(den - e_den, 1e-300) + U * r
            u = lamb_u(p[sl], m2[sl], v2[sl], wd, c1, c2, eps_)
            e_u = e_r + wd * ep[sl] + U * np.abs(wd * p[sl]) + U * np.abs(u)
            np_, nu = math.sqrt(sumsq(p[sl])), math.sqrt(sumsq(u))
            R, e_R = 1.0, 0.0
            if s.adapt and np_ > 0.0 and nu > 0.0:
                R = np_ / nu
                ne_p, ne_u = float(np.linalg.norm(ep[sl])), float(np.linalg.norm(e_u))
                e_R = (ne_p + R * ne_u) / max(nu - ne_u, 1e-300) + 2 * U * R
            st = lr_s * R
            e_st = lr_s * e_R + 2 * U * st
            e_p = ep[sl] + st * e_u + np.abs(u) * e_st + U * np.abs(st * u) + U * np.abs(p2[sl])
            self.ep[sl], self.em[sl], self.ev[sl] = self.SECOND * e_p, self.SECOND * e_m, self.SECOND * e_v
        return p2, m2, v2
