"""torch.optim.SGD's single-tensor update (dampening 0) restated in numpy, one operation per statement:

    d = g * grad_scale
    if weight_decay != 0:  d = d + weight_decay * p
    if momentum != 0:      buf = momentum * buf + d          (a zero buffer makes step 1 torch's buf = clone(d))
                           d = d + momentum * buf  if nesterov else  buf
    p = p - lr * d

Run in float32 — arrays and hyper-parameters alike, every product and every sum rounded on its own, numpy never fuses — this is
the BIT reference for ``avid_sgd_flat``; run in float64 with Python doubles it is the yardstick both are measured against."""
import numpy as np


def sgd_step(p, g, buf, lr, momentum, wd, nesterov=False, grad_scale=1.0, dtype=np.float32):
    """One step.  ``p`` / ``g`` / ``buf``: arrays of ``dtype`` (``buf`` None exactly when ``momentum == 0``).  Returns the new
    (p, buf); the inputs are left alone."""
    T = np.dtype(dtype).type
    lr, momentum, wd, grad_scale = T(lr), T(momentum), T(wd), T(grad_scale)
    assert p.dtype == g.dtype == np.dtype(dtype) and (buf is None) == (momentum == 0) and not (nesterov and momentum == 0)
    d = g * grad_scale
    if wd != 0:
        t = wd * p
        d = d + t
    if momentum != 0:
        t = momentum * buf
        buf = t + d
        if nesterov:
            t = momentum * buf
            d = d + t
        else:
            d = buf
    t = lr * d
    p = p - t
    assert p.dtype == np.dtype(dtype) and (buf is None or buf.dtype == np.dtype(dtype))
    return p, buf


def sgd_steps(p, grads, lr, momentum, wd, nesterov=False, grad_scale=1.0, dtype=np.float32, buf=None):
    """``len(grads)`` steps from ``p`` (and ``buf``, zeros if not given); inputs are cast to ``dtype`` first."""
    p = np.asarray(p).astype(dtype)
    if momentum != 0:
        buf = np.zeros_like(p) if buf is None else np.asarray(buf).astype(dtype)
    for g in grads:
        p, buf = sgd_step(p, np.asarray(g).astype(dtype), buf, lr, momentum, wd, nesterov, grad_scale, dtype)
    return p, buf
