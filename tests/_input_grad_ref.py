"""Float64 references and bars of the stems' input gradient (tests/test_input_grad_host.py, tests/test_gpu_input_grad.py).

Kernel level.  The reference is ``torch.nn.grad.conv3d_input`` on ``.double()`` tensors.  The per-element bar is

    |dx - dx64| <= 2 (K + 8) 2^-24 S,        K = 64 kt 16,

with S the same transposed convolution of |dy| and |w| in float64: K bounds the terms of one element (64 output channels,
kt frames, at most 4 x 4 taps of a stride-2 7 x 7 kernel), (K - 1) 2^-24 S is the first-order error of ANY order of summing
K float32 products, and the factor 2 and the + 8 leave room for the second-order terms and for products made of split
operands.  The second bar is the relative rms error, held to 3 x that of float32 torch on the CPU on the same data (what
tests/test_gpu_precision.py asks of the other kernels).  ``mutants`` gives the two controls that show the bars can fail.

Tower level.  ``video_tower`` / ``audio_tower`` restate ``models.R2Plus1D`` / ``models.Conv2D`` with ``conv3d``,
``batch_norm``, ``relu`` and ``max_pool3d`` of torch.nn.functional in the dtype of the state they are given; the bar on
d (pool * r).sum() / d input is a relative L2 error of 3 x that of the same restatement in float32 (ReLU and pooling ties
may flip between precisions, so no per-element bar)."""
import torch
import torch.nn.functional as F

VIDEO_SHAPES = [(1, 3, 1, 7, 9), (2, 3, 3, 17, 20), (3, 3, 2, 18, 21), (2, 3, 4, 32, 36), (1, 3, 5, 56, 60)]
AUDIO_SHAPES = [(3, 1, 9, 13), (2, 1, 50, 65), (1, 1, 200, 257)]
SHAPES = VIDEO_SHAPES + AUDIO_SHAPES
STRIDE = (1, 2, 2)


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def geometry(shape):
    """(x shape as [B,C,T,H,W], kernel, padding, y shape [B,64,To,Ho,Wo]) of the stem that reads an input of ``shape``."""
    if len(shape) == 4:                                   # the audio stem: Conv2d(1, 64, 7, 2, 3) as a T = kt = 1 Conv3d
        shape = (shape[0], shape[1], 1, shape[2], shape[3])
        k, pad = (1, 7, 7), (0, 3, 3)
    else:
        k, pad = (3, 7, 7), (1, 3, 3)
    out = tuple((n + 2 * p - kk) // s + 1 for n, p, kk, s in zip(shape[2:], pad, k, STRIDE))
    return shape, k, pad, (shape[0], 64) + out


_CASES = {}


def case(shape):
    """Inputs and references of one shape, made once and shared (never modified: callers copy).  dy is standard normal, w
    0.05 x standard normal; ``dx64`` the float64 reference, ``bound`` the per-element bar, ``dx32`` float32 torch on the CPU
    and ``rms32`` its relative rms error."""
    hit = _CASES.get(shape)
    if hit is None:
        xs, k, pad, ys = geometry(shape)
        g = torch.Generator().manual_seed(1000 + sum(v * (i + 1) for i, v in enumerate(shape)))
        dy = torch.randn(ys, generator=g)
        w = 0.05 * torch.randn((64, xs[1]) + k, generator=g)
        dx64 = dgrad(dy.double(), w.double(), xs, pad)
        S = dgrad(dy.double().abs(), w.double().abs(), xs, pad)
        K = 64 * k[0] * 16
        dx32 = dgrad(dy, w, xs, pad)
        hit = _CASES[shape] = dict(xs=xs, k=k, pad=pad, ys=ys, dy=dy, w=w, dx64=dx64, bound=2.0 * (K + 8) * 2.0 ** -24 * S, K=K,
                                   dx32=dx32, rms32=rel_rms(dx32, dx64))
    return hit


def dgrad(dy, w, xs, pad):
    return torch.nn.grad.conv3d_input(xs, w, dy, stride=STRIDE, padding=pad)


def rel_rms(got, ref):
    ref = ref.double()
    return float(((got.double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())


def bound_ratio(got, c):
    """max over elements of |got - dx64| / bound (<= 1: every element is inside the bar)."""
    err = (got.double() - c["dx64"]).abs()
    assert bool((c["bound"] > 0).all())
    return float((err / c["bound"]).max())


def mutants(c):
    """Float64 results of two wrong kernels: one that drops a tap (kt, kh, kw) for every channel, and one that drops the
    weight of ONE (output channel, tap) pair — of the 64 at that tap the one with the largest weight, so that the control
    does not hinge on a weight that happens to be near zero."""
    kt = c["k"][0] // 2
    w = c["w"].double()
    tap = w.clone()
    tap[:, :, kt, 3, 2] = 0
    one = w.clone()
    one[int(w[:, 0, kt, 2, 4].abs().argmax()), :, kt, 2, 4] = 0
    return {"dropped tap": dgrad(c["dy"].double(), tap, c["xs"], c["pad"]),
            "dropped weight": dgrad(c["dy"].double(), one, c["xs"], c["pad"])}


# ---------------------------------------------------------------------------------------------------------------- towers
def _bn(x, sd, name, train):
    return F.batch_norm(x, sd[name + ".running_mean"].clone(), sd[name + ".running_var"].clone(), sd[name + ".weight"],
                        sd[name + ".bias"], training=train, momentum=0.1, eps=1e-5)


def _w3(w):
    return w if w.dim() == 5 else w.unsqueeze(2)


def _cbr(x, sd, conv, bn, stride, pad, train, addend=None):
    y = F.conv3d(x, _w3(sd[conv + ".weight"]), stride=stride, padding=pad)
    if addend is not None:
        y = y + addend
    return F.relu(_bn(y, sd, bn, train))


def video_tower(x, sd, train, stages=("conv2x", "conv3x", "conv4x", "conv5x")):
    """models.R2Plus1D(10): x [B,3,T,H,W] -> pool [B,512,1,1,1]; ``sd``: its state_dict in the dtype to compute in."""
    h = _cbr(x, sd, "conv1.0", "conv1.1", (1, 2, 2), (1, 3, 3), train)
    h = F.max_pool3d(h, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    for n, name in enumerate(stages):
        s = (1, 1, 1) if n == 0 else (2, 2, 2)
        res = F.conv3d(h, sd[name + ".res_conv.weight"], stride=s) if name + ".res_conv.weight" in sd else h
        h = _cbr(h, sd, name + ".spt_conv1", name + ".spt_bn1", (1, s[1], s[2]), (0, 1, 1), train)
        h = _cbr(h, sd, name + ".tmp_conv1", name + ".tmp_bn1", (s[0], 1, 1), (1, 0, 0), train)
        h = _cbr(h, sd, name + ".spt_conv2", name + ".spt_bn2", (1, 1, 1), (0, 1, 1), train)
        h = _cbr(h, sd, name + ".tmp_conv2", name + ".out_bn", (1, 1, 1), (1, 0, 0), train, addend=res)
    return h.amax(dim=(2, 3, 4), keepdim=True)


def audio_tower(x, sd, train):
    """models.Conv2D(): x [B,1,T,F] -> pool [B,512,1,1]."""
    h = _cbr(x.unsqueeze(2), sd, "conv1.0", "conv1.1", (1, 2, 2), (0, 3, 3), train)
    for name, s in (("block1", 2), ("block2", 2), ("block3", 2), ("block4", 1)):
        h = _cbr(h, sd, name + ".conv1", name + ".bn1", (1, s, s), (0, 1, 1), train)
        h = _cbr(h, sd, name + ".conv2", name + ".bn2", (1, 1, 1), (0, 1, 1), train)
    return h.amax(dim=(2, 3, 4)).unsqueeze(-1).unsqueeze(-1)


def tower_input_grad(tower, x, sd, r, train, dtype):
    """d (tower(x) * r).sum() / dx in ``dtype`` on the CPU, with the parameter gradients ({name: grad}) when ``train``."""
    sd = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu() for k, v in sd.items()}
    names = [k for k in sd if sd[k].is_floating_point() and "running" not in k]
    if train:
        for k in names:
            sd[k].requires_grad_(True)
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    loss = (tower(xd, sd, train) * r.detach().cpu().to(dtype)).sum()
    grads = torch.autograd.grad(loss, [xd] + ([sd[k] for k in names] if train else []))
    return grads[0], dict(zip(names, grads[1:]))


def rel_l2(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).norm() / ref.norm())
