"""The stems' input gradients (``stem_dgrad_kernel``): d/d clip and d/d spectrogram, from the kernel up to ``AV_Wrapper``.

Kernel: every element inside the float64 bound of tests/_input_grad_ref.py and a relative rms error of at most 3 x float32
torch's on the CPU (measured here, on the same data), the kernel named in the launch log, the same bits on a second run and
under CU budgets of 8 and 24, nothing written outside dx (tests/_guards.py).  Autograd: ``ops.conv_cl(...,
channel_first=True)`` gives dx with or without dw, and dw does not change.  Towers: d (pool * r).sum() / d input against the
float64 restatement, to 3 x the float32 restatement's own relative L2 error.  ``AV_Wrapper``: both input gradients in eval
mode, and the per-layer path (not the launch programs, which stop at the stems' weight gradients) in train mode."""
import copy
import ctypes as C

import pytest
import torch

import _input_grad_ref as R
from _guards import FILLS, guarded

pytestmark = pytest.mark.gpu


def _weight(w, dev):
    """The parameter's memory [64][kt][7][7][Cin] (audio: 4-D, as models.Conv2D holds it) on the device."""
    from avid_hip import ops
    if w.shape[2] == 1 and w.shape[1] == 1:
        w = w[:, :, 0]
    out = ops.make_weight(*w.shape)
    out.copy_(w)
    return out.to(dev)


def _dgrad(c, dy_cl, w_dev, place=None, ws_exact=False):
    """``avid_conv_dgrad`` of a channel-first stem descriptor: dx [B,Cin,Ti,Hi,Wi], pre-filled with NaN."""
    from avid_hip import lib, ops
    B, cin, Ti, Hi, Wi = c["xs"]
    d = ops._desc_cached((B, Ti, Hi, Wi), cin, 64, c["k"], R.STRIDE, c["pad"], True)[0]
    assert lib.raw("avid_conv_dgrad_bn_rows")(C.byref(d)) == 0
    nb = lib.raw("avid_conv_dgrad_workspace_bytes")(C.byref(d))
    dx = torch.empty(c["xs"], dtype=torch.float32, device=dy_cl.device)
    if place is None:
        dx.fill_(float("nan"))
    ws = ops.workspace(dy_cl.device, nb) if ws_exact else None
    lib.call("avid_conv_dgrad", C.byref(d), ops._p(dy_cl), ops._p(w_dev), None, None, None, None, ops._p(dx), None,
             ops._p(ws), nb if ws_exact else 0, ops._stream())
    return dx


def _device_case(shape, dev):
    c = R.case(shape)
    return c, c["dy"].permute(0, 2, 3, 4, 1).contiguous().to(dev), _weight(c["w"], dev)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_kernel_against_float64(shape, gpu_device, kernel_log):
    from avid_hip import ops
    c, dy, w = _device_case(shape, gpu_device)
    with kernel_log() as log:
        dx = _dgrad(c, dy, w)
    name = f"stem_dgrad_kernel<{c['xs'][1]},{c['k'][0]}>"
    assert log.launches(name) == 1, sorted(log.report)
    got = dx.cpu()
    assert bool(torch.isfinite(got).all()), "an element of dx was not written"
    ratio, rms = R.bound_ratio(got, c), R.rel_rms(got, c["dx64"])
    print(f"{R.shape_id(shape)}: {ratio:.2e} of the bound (float32 torch {R.bound_ratio(c['dx32'], c):.2e}), "
          f"relative rms {rms:.2e} (float32 torch {c['rms32']:.2e})")
    assert ratio <= 1.0
    assert rms <= 3.0 * c["rms32"]
    # the same bits on a second run and under every CU budget
    assert torch.equal(_dgrad(c, dy, w).cpu().view(torch.int32), got.view(torch.int32))
    full = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    try:
        for cus in (8, 24):
            if cus < full:
                assert ops.set_cu_budget(cus) == cus
            assert torch.equal(_dgrad(c, dy, w).cpu().view(torch.int32), got.view(torch.int32)), f"CU budget {cus}"
    finally:
        ops.set_cu_budget(0)


def test_unsupported_channel_first_geometry_is_refused_before_a_launch(gpu_device):
    from avid_hip import lib, ops
    d = ops._desc((2, 4, 16, 16), 3, 64, (3, 5, 5), (1, 2, 2), (1, 2, 2), True)
    buf = torch.zeros(1 << 16, device=gpu_device)
    assert lib.raw("avid_conv_dgrad_workspace_bytes")(C.byref(d)) == 0
    rc = lib.raw("avid_conv_dgrad")(C.byref(d), ops._p(buf), ops._p(buf), None, None, None, None, ops._p(buf), None, None, 0,
                                    ops._stream())
    assert rc == -4 and "channel-first" in lib.last_error()           # AVID_E_UNSUPPORTED
    c = R.case((1, 3, 1, 7, 9))
    d = ops._desc_cached((1, 1, 7, 9), 3, 64, c["k"], R.STRIDE, c["pad"], True)[0]
    rc = lib.raw("avid_conv_dgrad")(C.byref(d), ops._p(buf), ops._p(buf), ops._p(buf), None, None, None, ops._p(buf), None, None, 0,
                                    ops._stream())
    assert rc == -1                                                    # AVID_E_BADARG: wt must be NULL
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


@pytest.mark.parametrize("shape", [(2, 3, 3, 17, 20), (2, 1, 50, 65)], ids=R.shape_id)
def test_guarded_call_writes_dx_and_nothing_else(shape, gpu_device):
    c, dy, w = _device_case(shape, gpu_device)
    plain = _dgrad(c, dy, w).cpu().view(torch.int32)
    for fill in FILLS:
        with guarded(fill) as g:
            dx = _dgrad(c, g.place(dy), g.place(w), place=g.place, ws_exact=True)
            torch.cuda.synchronize()
            g.check()
            got = dx.cpu().view(torch.int32)
        assert sum(r.kind == "input" for r in g.records) == 2 and [a for a, _, _ in g.workspaces] == [0]
        assert 0 in g.size_values
        assert torch.equal(got, plain), f"fill 0x{fill:02X}"


# ---------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("shape", [(2, 3, 3, 17, 20), (3, 3, 2, 18, 21), (2, 1, 50, 65)], ids=R.shape_id)
def test_autograd_returns_dx_with_and_without_dw(shape, gpu_device):
    from avid_hip import ops
    c, dy, w = _device_case(shape, gpu_device)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(c["xs"], generator=g).to(gpu_device)

    def run(x_grad, w_grad):
        xd, wd = x.clone().requires_grad_(x_grad), w.detach().clone().requires_grad_(w_grad)
        assert ops.weight_layout_ok(wd)
        y = ops.conv_cl(xd, wd, R.STRIDE, c["pad"], channel_first=True)
        return torch.autograd.grad(y, [t for t, on in ((xd, x_grad), (wd, w_grad)) if on], dy)

    dx, dw = run(True, True)
    (dw_alone,) = run(False, True)
    (dx_alone,) = run(True, False)            # the saliency set-up: the weight frozen
    assert dx.shape == x.shape and dx.is_contiguous()
    assert torch.equal(dw.view(torch.int32), dw_alone.view(torch.int32))
    assert torch.equal(dx.view(torch.int32), dx_alone.view(torch.int32))
    assert R.bound_ratio(dx.cpu(), c) <= 1.0 and R.rel_rms(dx.cpu(), c["dx64"]) <= 3.0 * c["rms32"]


# ------------------------------------------------------------------------------------------------------------------ towers
def _tower(kind, dev):
    import models
    torch.manual_seed(11)
    if kind == "video":
        m, x, ref = models.R2Plus1D(10), torch.randn(2, 3, 4, 32, 32), R.video_tower
    else:
        m, x, ref = models.Conv2D(), torch.randn(2, 1, 40, 33), R.audio_tower
    with torch.no_grad():                    # running statistics and affine maps off their initial values
        for mod in m.modules():
            if hasattr(mod, "running_var"):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
    r = torch.randn(2, 512, *([1] * (x.dim() - 2)))
    return m.to(dev), x, r, ref


def _state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("kind", ["video", "audio"])
def test_tower_input_gradient_eval_all_frozen(kind, gpu_device):
    m, x, r, ref = _tower(kind, gpu_device)
    m.eval().requires_grad_(False)
    sd = _state(m)
    xd = x.to(gpu_device).requires_grad_(True)
    (dx,) = torch.autograd.grad((m(xd) * r.to(gpu_device)).sum(), xd)
    (dx2,) = torch.autograd.grad((m(xd) * r.to(gpu_device)).sum(), xd)
    dx64, _ = R.tower_input_grad(ref, x, sd, r, False, torch.float64)
    dx32, _ = R.tower_input_grad(ref, x, sd, r, False, torch.float32)
    e, e32 = R.rel_l2(dx, dx64), R.rel_l2(dx32, dx64)
    print(f"{kind} tower, eval: relative L2 error {e:.2e} (float32 restatement {e32:.2e})")
    assert dx.shape == x.shape and float(dx64.norm()) > 0
    assert e <= 3.0 * e32
    assert torch.equal(dx.view(torch.int32), dx2.view(torch.int32))


def test_video_tower_input_gradient_train_mode(gpu_device):
    m, x, r, ref = _tower("video", gpu_device)
    m.train()
    sd = _state(m)
    m2 = copy.deepcopy(m)
    params = [p for p in m.parameters()]
    xd = x.to(gpu_device).requires_grad_(True)
    grads = torch.autograd.grad((m(xd) * r.to(gpu_device)).sum(), [xd] + params)
    grads2 = torch.autograd.grad((m2(x.to(gpu_device)) * r.to(gpu_device)).sum(), list(m2.parameters()))
    for (n, _), g1, g2 in zip(m.named_parameters(), grads[1:], grads2):
        assert torch.equal(g1.contiguous().view(torch.int32), g2.contiguous().view(torch.int32)), n
    dx64, _ = R.tower_input_grad(ref, x, sd, r, True, torch.float64)
    dx32, _ = R.tower_input_grad(ref, x, sd, r, True, torch.float32)
    e, e32 = R.rel_l2(grads[0], dx64), R.rel_l2(dx32, dx64)
    print(f"video tower, train: relative L2 error {e:.2e} (float32 restatement {e32:.2e})")
    assert float(dx64.norm()) > 0
    assert e <= 3.0 * e32


# -------------------------------------------------------------------------------------------------------------- AV_Wrapper
def _wrapper(dev):
    import models
    torch.manual_seed(13)
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).to(dev)
    return m, torch.randn(2, 3, 8, 64, 64, device=dev), torch.randn(2, 1, 40, 100, device=dev)


def test_av_wrapper_eval_input_gradients(gpu_device):
    m, video, audio = _wrapper(gpu_device)
    m.eval().requires_grad_(False)

    def run():
        v, a = video.clone().requires_grad_(True), audio.clone().requires_grad_(True)
        ve, ae = m(v, a)
        (ve * ae).sum().backward()
        return v.grad, a.grad

    gv, ga = run()
    gv2, ga2 = run()
    for g, x, g2 in ((gv, video, gv2), (ga, audio, ga2)):
        assert g is not None and g.shape == x.shape
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert torch.equal(g.view(torch.int32), g2.view(torch.int32))


def test_av_wrapper_train_input_gradient_takes_the_per_layer_path(gpu_device):
    m, video, audio = _wrapper(gpu_device)
    m.train()
    v = video.clone().requires_grad_(True)
    ve, ae = m(v, audio)
    assert not type(ve.grad_fn).__name__.startswith("NetFn"), type(ve.grad_fn).__name__
    (ve * ae).sum().backward()
    assert v.grad is not None and v.grad.shape == video.shape
    assert bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0
    assert all(p.grad is not None for p in m.parameters())
