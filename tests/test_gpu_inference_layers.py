"""The kernels of the inference programs, one by one, against the launches they replace.

* ``avid_conv_fwd_out`` — conv2x's temporal layers (tconv64_kernel) with the eval-mode BatchNorm (+ReLU) of their OUTPUT in the
  epilogue — must give the bits of ``avid_conv_fwd[_in]`` followed by ``avid_bn_fwd_eval(save4)``: it is the same fma on the same
  fp32 value.  Shapes as tests/test_gpu_tconv.py found necessary: a ragged last tile, tiles that straddle clips, fewer positions
  than one tile.  ``ops.tconv_configure(2)`` sends these small shapes through the kernel (the default rule asks for three rounds
  of tiles for the CUs).
* the same layer against float64, with no bit-identity shortcut.
* what the entry point refuses.
* the eval-mode stem tail, the batched coefficient launch and the apply pass against the calls they stand for.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detgen

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4           # include/avid_hip.h: AVID_E_UNSUPPORTED


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture
def tconv_all(gpu_device):
    from avid_hip import ops
    assert ops.tconv_configure(2) == 2
    yield
    ops.tconv_configure(-1)


def _bn(tag, Cc, dev=None):
    """gamma, beta, running_mean, running_var of one BatchNorm: a third of the scales negative, shifts that put about half of
    a unit-variance input at or below zero."""
    gamma = T(detgen.det_uniform(f"{tag}:gamma", (Cc,))).float() + 0.3             # [-0.7, 1.3)
    beta = T(detgen.det_uniform(f"{tag}:beta", (Cc,))).float() * 0.3
    rm = T(detgen.det_normalish(f"{tag}:rm", (Cc,))).float() * 0.2
    rv = T(detgen.det_uniform(f"{tag}:rv", (Cc,))).float() * 0.75 + 1.0            # [0.25, 1.75)
    out = [gamma, beta, rm, rv]
    return [t.to(dev) for t in out] if dev is not None else out


def _bn_eval(x, bn, relu):
    """avid_bn_fwd_eval with save4: the normalised tensor and the [4][C] vectors."""
    from avid_hip import lib, ops
    Cc = x.shape[-1]
    y = torch.empty_like(x)
    s4 = torch.empty((4, Cc), dtype=torch.float32, device=x.device)
    lib.call("avid_bn_fwd_eval", x.numel() // Cc, Cc, ops._p(x), *[ops._p(t) for t in bn], 1e-5, int(relu), ops._p(y), ops._p(s4),
             ops._stream())
    return y, s4


def _weight(tag, dev, *shape):
    from avid_hip import ops
    w = ops.make_weight(*shape)
    w.copy_(T(detgen.det_param(f"{tag}.weight", shape)))
    return w.to(dev)


SHAPES = [(3, 13, 15), (9, 20, 20), (1, 3, 5)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_out_affine_is_conv_then_bn_eval(shape, gpu_device, tconv_all):
    """Every combination of {ReLU, addend, input-side map} x the three tile geometries: torch.equal with the unfused pair, and
    the launch counter says that the fused form ran."""
    from avid_hip import lib, ops
    B, Hi, Wi = shape
    dev = gpu_device
    x = T(detgen.det_normalish(f"oaff:{shape}:x", (B, 8, Hi, Wi, 64))).to(dev)
    add = T(detgen.det_normalish(f"oaff:{shape}:add", (B, 8, Hi, Wi, 64))).to(dev)
    w = _weight(f"oaff:{shape}:w", dev, 64, 64, 3, 1, 1)
    bn_in, bn_out = _bn(f"oaff:{shape}:in", 64, dev), _bn(f"oaff:{shape}:out", 64, dev)
    _, s4_in = _bn_eval(x, bn_in, True)
    count = lib.raw("avid_debug_out_affine_launches")
    stride, pad = (1, 1, 1), (1, 0, 0)
    for in_map in (False, True):
        for addend in (None, add):
            if in_map:
                raw = ops.conv_fwd_in(x, w, stride, pad, s4_in[2], s4_in[3], relu=True, addend=addend)
            else:
                raw = ops.conv_cl(x, w, stride, pad, addend=addend)
            for relu in (False, True):
                want, s4 = _bn_eval(raw, bn_out, relu)
                n0 = count()
                got = ops.conv_fwd_out(x, w, stride, pad, s4[2], s4[3], out_relu=relu, addend=addend,
                                       in_scale=s4_in[2] if in_map else None, in_shift=s4_in[3] if in_map else None, in_relu=True)
                assert count() == n0 + 1, "the fused form did not run"
                assert torch.equal(got, want), (in_map, addend is not None, relu, float((got - want).abs().max()))
                if relu:      # the shifts do put a good part of the values at zero (the max() is exercised)
                    frac = float((want == 0).float().mean())
                    assert 0.2 < frac < 0.8, frac


def test_conv_out_affine_vs_float64(gpu_device, tconv_all):
    """conv -> eval BatchNorm -> ReLU at (9, 20, 20) against the float64 composite.  Bar (tests/test_gpu_precision.py's form): rms
    error / rms(output) at most 3x that of the same composite in float32 by torch on the CPU.
    Measured on an MI355X: device 1.98e-7, host float32 1.35e-7 (ratio 1.47)."""
    from avid_hip import ops
    B, Hi, Wi = 9, 20, 20
    x = T(detgen.det_normalish("oaff64:x", (B, 64, 8, Hi, Wi)))
    w = T(detgen.det_param("oaff64:w.weight", (64, 64, 3, 1, 1)))
    gamma, beta, rm, rv = _bn("oaff64:bn", 64)

    def composite(dt):
        y = F.conv3d(x.to(dt), w.to(dt), stride=1, padding=(1, 0, 0))
        return F.relu(F.batch_norm(y, rm.to(dt), rv.to(dt), gamma.to(dt), beta.to(dt), False, 0.0, 1e-5))
    want, host = composite(torch.float64), composite(torch.float32)
    dev = gpu_device
    wd = ops.make_weight(64, 64, 3, 1, 1)
    wd.copy_(w)
    s4 = ops.bn_eval_coeffs([(gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), 1e-5)])[0]
    got = ops.conv_fwd_out(x.permute(0, 2, 3, 4, 1).contiguous().to(dev), wd.to(dev), (1, 1, 1), (1, 0, 0), s4[2], s4[3], out_relu=True)
    got = got.permute(0, 4, 1, 2, 3).cpu()

    def rms_rel(a):
        return float(((a.double() - want) ** 2).mean().sqrt() / (want ** 2).mean().sqrt())
    e_dev, e_host = rms_rel(got), rms_rel(host)
    print(f"out-affine layer vs float64: device {e_dev:.3e}, host float32 {e_host:.3e}, ratio {e_dev / e_host:.2f}")
    assert e_dev <= 3.0 * e_host, (e_dev, e_host)


def test_conv_out_affine_refusals(gpu_device, tconv_all):
    """avid_conv_takes_out_affine is 0 for 7 or 32 frames, 128 channels, stride 2 and (1,3,3); avid_conv_fwd_out answers
    AVID_E_UNSUPPORTED there, and for a layer that takes it when BatchNorm partial sums are requested."""
    from avid_hip import lib, ops
    dev = gpu_device
    takes = lib.raw("avid_conv_takes_out_affine")
    fwd = lib.raw("avid_conv_fwd_out")

    def attempt(xs, cin, cout, k, stride, pad, partials=False):
        d = ops._desc_cached(xs, cin, cout, k, stride, pad, False)[0]
        x = torch.zeros(xs + (cin,), device=dev)
        w = _weight("oaffref:w", dev, cout, cin, *k)
        y = torch.zeros((xs[0], d.To, d.Ho, d.Wo, cout), device=dev)
        s4 = torch.ones((4, cout), device=dev)
        part = torch.zeros((4096, 2, cout), device=dev) if partials else None
        u = ops._fwd_u(w, d) if d.split_fwd else torch.zeros(6 * w.numel(), dtype=torch.uint8, device=dev)
        out = lib.OutAffine(s4[2].data_ptr(), s4[3].data_ptr(), 1)
        ws = ops.workspace(dev, 1 << 20)
        rc = fwd(C.byref(d), ops._p(x), None, ops._p(w), ops._p(u), None, None, 0, C.byref(out), ops._p(y), ops._p(part), ops._p(ws),
                 ws.numel(), ops._stream())
        return int(takes(C.byref(d))), rc

    t, s1, p = (3, 1, 1), (1, 1, 1), (1, 0, 0)
    assert attempt((2, 8, 6, 6), 64, 64, t, s1, p) == (1, 0)
    assert attempt((2, 8, 6, 6), 64, 64, t, s1, p, partials=True) == (1, UNSUPPORTED)
    assert "partial" in lib.last_error()
    for xs, cin, cout, k, stride, pad in (((2, 7, 6, 6), 64, 64, t, s1, p), ((2, 32, 6, 6), 64, 64, t, s1, p),
                                          ((2, 8, 6, 6), 128, 128, t, s1, p), ((2, 8, 6, 6), 64, 64, t, (2, 1, 1), p),
                                          ((2, 8, 6, 6), 64, 64, (1, 3, 3), s1, (0, 1, 1))):
        assert attempt(xs, cin, cout, k, stride, pad) == (0, UNSUPPORTED), (xs, cin, k, stride)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(2, 8, 20, 20, 64), (1, 3, 9, 11, 64)], ids=lambda s: "x".join(map(str, s)))
def test_stem_tail_eval_is_bn_eval_then_maxpool(shape, gpu_device):
    """One pass against the two launches, values only (no argmax is written): signed zeros and ties included — the input holds
    exact zeros and exact repeats, and a channel whose scale is zero."""
    from avid_hip import ops
    dev = gpu_device
    x = T(detgen.det_normalish(f"tail:{shape}:x", shape)).float()
    x[:, :, ::3, 1::2] = 0.0                              # zeros (with negative scales: -0.0 products) ...
    x[:, :, 1::4] = x[:, :, 0:1].expand_as(x[:, :, 1::4])      # ... and rows repeated: ties inside a window
    x = x.to(dev).contiguous()
    bn = _bn(f"tail:{shape}:bn", shape[-1], dev)
    bn[0][5] = 0.0
    y, s4 = _bn_eval(x, bn, True)
    want = ops.maxpool_hw3s2(y)
    got = ops.bn_relu_maxpool_eval(x, s4[2], s4[3])
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(torch.signbit(got), torch.signbit(want))


def test_batched_coefficients_are_the_per_layer_vectors(gpu_device):
    """One table with C = 64, 128, 256, 512 (eps 1e-5): every [4][C] block equals avid_bn_fwd_eval's save4."""
    from avid_hip import ops
    dev = gpu_device
    bns = [_bn(f"coef:{Cc}", Cc, dev) for Cc in (64, 128, 256, 512)]
    got = ops.bn_eval_coeffs([tuple(bn) + (1e-5,) for bn in bns])
    for bn, g in zip(bns, got):
        Cc = bn[0].numel()
        x = T(detgen.det_normalish(f"coef:{Cc}:x", (3, Cc))).to(dev)
        y, s4 = _bn_eval(x, bn, False)
        assert torch.equal(g, s4), Cc
        assert torch.equal(ops.bn_apply_eval(x, g[2], g[3], relu=False), y)
        assert torch.equal(ops.bn_apply_eval(x, g[2], g[3], relu=True), _bn_eval(x, bn, True)[0])


def test_tconv_configure_drops_the_cached_answers(gpu_device):
    """ops.tconv_configure: a layer's in_affine / out_affine answer is re-asked after the switch moved, and the epoch the compiled
    programs are keyed by moves with it."""
    from avid_hip import ops
    geo = ((2, 8, 6, 6), 64, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), False)
    try:
        ops.tconv_configure(0)
        e0 = ops.wino_epoch()
        assert not ops._desc_cached(*geo)[0].out_affine and not ops._desc_cached(*geo)[0].in_affine
        assert ops.tconv_configure(2) == 2 and ops.wino_epoch() > e0
        assert ops._desc_cached(*geo)[0].out_affine and ops._desc_cached(*geo)[0].in_affine
    finally:
        ops.tconv_configure(-1)
    assert not ops._desc_cached(*geo)[0].out_affine        # 5 tiles: the default rule asks for three rounds of the CUs
