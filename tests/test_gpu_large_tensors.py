"""The kernels on tensors of 2^31 bytes, 2^32 bytes and 2^31 elements — the route the library takes from 2 GiB per tensor on
(DESIGN.md "Tensors of 2 GiB and more"): no Winograd, no tconv64 / twgrad64, strided input gradients on igemm_kernel<..,true>,
re-based buffer descriptors, ``long long`` indices in the stems and in csrc/norm_pool.hip.

Shapes, probe items and checkers: tests/_large_ref.py (pinned, and turned on planted defects, by
tests/test_large_tensors_host.py).  Every case runs the four checks described there; the big tensors are filled on the device.
Each test states its peak device memory and skips only when ``torch.cuda.mem_get_info`` shows less than that.

Bars are the project's: convolutions 2e-5 of max|ref| for y and dx and 5e-5 for dw (tests/test_gpu_ops.py), BatchNorm mean /
running mean 1e-6, invstd / y / running variance 1e-5, dx / dgamma / dbeta 2e-5, colsum 1e-6 (tests/test_gpu_bs64_norm.py),
pooled values bit-equal and the routing rule rtol 1e-6, atol 1e-7 (test_maxpool_hw3s2).  The sums over 8 to 34 M rows print
their error against the float64 accumulation next to that of a float32 torch reduction of the same data before they assert.

Measured on an MI355X (relative to max|float64 reference|; in brackets the float32 torch reduction of the same data).  No bar had
to be set: every inherited one holds.
  dense weight gradients, 8.4 M rows:  spatial 1.0e-5 (1.8e-6), temporal 6.8e-6 / 6.4e-6 (1.8e-6), strided 4.5e-6 (8.3e-7),
      strided wide 5.7e-6 (6.6e-7), video stem 3.1e-6 (6.9e-7), audio stem 3.0e-6 (8.6e-7); 16.9 M rows: spatial 1.6e-5 (1.9e-6),
      video stem 4.9e-6 (7.9e-7) -- bar 5e-5; with dy on the probe items only <= 1.6e-6
  y and dx of the convolutions: <= 0.07 of 2e-5 on the probe items, <= 0.11 of 2e-5 against the chunked runs
  BatchNorm over 8.4 / 16.9 / 33.7 M rows: mean 5.2e-8 / 5.2e-8 / 5.3e-8 (1.1e-7 / 1.2e-7 / 1.9e-7) of 1e-6, invstd 5e-8 (0.8-1.4e-7),
      running mean <= 7.6e-8, running variance <= 8.9e-8, y 8.8e-8, dx <= 2.5e-7, dgamma <= 4.2e-7, dbeta <= 6.0e-7 (4.3e-7 ... 6.2e-7)
  colsum over 8.4 / 16.9 / 33.7 M rows: 3.4e-7 / 3.7e-7 / 3.3e-7 (3.7e-7 / 3.7e-7 / 5.0e-7) of 1e-6 -- one running fp32 sum per lane,
      as the kernel did before, was at 3.1e-5
  kernels in the launch log: igemm_pk_kernel<4,1,1,2,0|1> (+ splitk_reduce_kernel), wgrad_tab_kernel<1,3> / <2,2>, igemm_pk_kernel<4,1,1,4,0>,
      igemm_kernel<4,1,1,2,1>s2 (64 -> 128), igemm_kernel<2,2,2,2,1>s2 (128 -> 256), stem_fwd3p / stem_fwd / stem_dgrad / stem_wgrad
  peak device memory: 8.8 ... 24.5 GiB (convolutions), 7.8 ... 42.8 GiB (norm / pool at B = 21500)"""
import ctypes as C
import gc

import pytest
import torch
import torch.nn.functional as F

import _large_ref as R
from _guards import guarded

pytestmark = pytest.mark.gpu

GIB = 1 << 30
BAR_Y, BAR_DX, BAR_DW = 2e-5, 2e-5, 5e-5
BAR = {"mean": 1e-6, "invstd": 1e-5, "y": 1e-5, "running_mean": 1e-6, "running_var": 1e-5, "dx": 2e-5, "dgamma": 2e-5,
       "dbeta": 2e-5, "colsum": 1e-6}


@pytest.fixture(autouse=True)
def _free_after_each_case():
    yield
    gc.collect()
    if torch.cuda.is_available():
        from avid_hip import ops
        ops._WS.clear()                     # the shared scratch grew with the chunked runs (up to 8 dx-shaped slabs): it is re-made on demand
        torch.cuda.empty_cache()


def _need(dev, gib):
    """Skip only when the device does not have ``gib`` GiB free (every figure below is under 64)."""
    assert gib < 64
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < gib * GIB:
        pytest.skip(f"needs {gib} GiB of device memory, {free / GIB:.1f} free")
    torch.cuda.reset_peak_memory_stats(dev)
    _BASE[0] = torch.cuda.memory_allocated(dev)       # what earlier tests of the session still hold (fixtures, cached scratch)


_BASE = [0]


def _peak(dev, gib, what):
    peak = (torch.cuda.max_memory_allocated(dev) - _BASE[0]) / GIB
    print(f"  {what}: peak device memory {peak:.1f} GiB (stated need {gib})")
    assert peak <= gib, (what, peak, gib)


def _show(what, err, bar, f32=None):
    extra = "" if f32 is None else f"   float32 torch reduction {f32:.2e}"
    print(f"  {what:44s} {err:.2e} / {bar:.0e} = {err / bar:5.2f} of the bar{extra}")
    return err


def _workspaces_exact(g):
    for asked, site, _ in g.workspaces:
        assert asked in g.size_values, f"workspace of {asked} bytes at {site}; the size functions said {sorted(g.size_values)}"


# ================================================================================================================ convolutions
# peak memory: x, y, dy, dx + the chunks' dx + the sparse run's y + chunk temporaries; stated per case in GiB (the strided cases:
# + the 8 dx-shaped K-split slabs, 8 GiB, of a chunk that runs on the persistent kernel)
CONV_NEED = {("spatial", 5400): 16, ("temporal", 5000): 16, ("temporal_13x15", 5378): 16, ("strided", 5400): 24,
             ("strided_wide", 10800): 24, ("video_stem", 22000): 12, ("audio_stem", 52500): 12, ("spatial", 10800): 30,
             ("video_stem", 44000): 20, ("spatial", 21500): 24}


def _conv_case(layer, B, dev, kernel_log, grads=True):
    from avid_hip import lib, ops
    cin, cout, k, s, p, thw, cf = R.LAYERS[layer]
    need = CONV_NEED[(layer, B)]
    _need(dev, need)
    ib = R.item_bytes(layer)
    items = R.probe_items(B, ib, seed=1)
    To, Ho, Wo = R.out_extent(layer)
    w = R.weight(layer, 11)
    wd = ops.make_weight(cout, cin, *k)
    wd.copy_(w)
    wd = wd.to(dev)
    x = R.fill((B, cin) + thw if cf else (B,) + thw + (cin,), 21, dev)
    dy = R.fill((B, To, Ho, Wo, cout), 22, dev, kind="uniform") if grads else None
    d = ops._desc((B,) + thw, cin, cout, k, s, p, cf)
    tag = f"{layer} B={B}"
    print(f"\n{tag}: x {B * ib[0] / 1e9:.2f} GB, y {B * ib[1] / 1e9:.2f} GB, probe items {items}")

    # ---- the dense run: default dispatch, guarded (check 4), launch log
    with guarded(0xFF) as g:
        with kernel_log() as log:
            xr, wr = x.detach().requires_grad_(grads), wd.detach().requires_grad_(grads)
            y = ops.conv_cl(xr, wr, s, p, channel_first=cf)
            dx = dw = None
            if grads:
                dx, dw = torch.autograd.grad(y, [xr, wr], dy)
        g.check()
        _workspaces_exact(g)
    y = y.detach()
    print(f"  kernels: {sorted(log.report)}")
    for prefix in ("wino", "tconv64", "twgrad64"):
        assert log.launches(prefix) == 0, (prefix, sorted(log.report))
    if layer.startswith("strided") and grads:
        buf = C.create_string_buffer(256)
        assert lib.raw("avid_conv_kernel_name")(C.byref(d), 1, buf, 256) == 0
        said = buf.value.decode().split(" ")[0]
        assert said.startswith("igemm_kernel<") and said.endswith(",1>s2"), said
        assert log.launches("igemm_kernel<") == 1 and log.launches(said) == 1, (said, sorted(log.report))
        assert log.launches("igemm_pk_kernel<4,1,1,2,1>s2") + log.launches("igemm_pk_kernel<2,2,2,2,1>s2") == 0
        if layer == "strided":
            assert said == "igemm_kernel<4,1,1,2,1>s2"
    elif cf:
        assert log.launches("stem_fwd") == 1, sorted(log.report)
        assert not grads or (log.launches("stem_dgrad_kernel") == 1 and log.launches("stem_wgrad") >= 1), sorted(log.report)
    else:
        assert log.launches("igemm_pk_kernel<") == (2 if grads else 1), sorted(log.report)
        assert not grads or log.launches("wgrad_tab_kernel") >= 1, sorted(log.report)
    R.assert_written(y, tag + " y")
    if grads:
        R.assert_written(dx, tag + " dx")
        R.assert_written(dw, tag + " dw")

    # ---- check 1: probe items against float64 on the CPU
    refs = {i: R.conv_item64(layer, x[i], w, dy[i] if grads else None) for i in items}
    share = {"y": R.check_probes(y, lambda i: refs[i][0], items, BAR_Y, tag + " y")}
    if grads:
        share["dx"] = R.check_probes(dx, lambda i: refs[i][1], items, BAR_DX, tag + " dx")

    # ---- check 2: the whole tensor against runs on chunks below 1 GiB (convolutions: 2e-5 of the chunk's largest value)
    n = R.chunk_items(ib)
    chunk_out = {}

    def run_chunk(b0, b1):
        xc, wc = x[b0:b1].detach().requires_grad_(grads), wd.detach().requires_grad_(grads)
        yc = ops.conv_cl(xc, wc, s, p, channel_first=cf)
        if grads:
            dxc, dwc = torch.autograd.grad(yc, [xc, wc], dy[b0:b1])
            chunk_out[b0] = (dxc, dwc.double())
        return yc.detach()

    share["y vs chunks"] = R.check_chunks(y, run_chunk, n, BAR_Y, tag + " y")
    if grads:
        share["dx vs chunks"] = R.check_chunks(dx, lambda b0, b1: chunk_out[b0][0], n, BAR_DX, tag + " dx")
        dw_chunks = sum(v[1] for v in chunk_out.values())
        chunk_out.clear()

        # ---- check 3: the weight gradient.  Dense: against a float64 accumulation on the device, next to a float32 torch
        # reduction of the same data and to the sum of the chunked runs
        dw64 = R.wgrad64(layer, x, dy)
        dw32 = R.wgrad64(layer, x, dy, dtype=torch.float32)
        e32 = R.relerr(dw32, dw64)
        share["dw dense"] = _show(tag + " dw vs float64 on the device", R.relerr(dw, dw64), BAR_DW, e32) / BAR_DW
        _show(tag + " sum of the chunks' dw vs float64", R.relerr(dw_chunks, dw64), BAR_DW)
        assert R.relerr(dw, dw64) < BAR_DW and R.relerr(dw_chunks, dw64) < BAR_DW
        del dw64, dw32, dx
        # sparse: dy non-zero on the probe items only, x fully random (a wrong read shows) — float64 on the CPU over those items
        keep = dy[items].clone()
        dy.zero_()
        dy[items] = keep
        wr = wd.detach().requires_grad_(True)
        (dw_s,) = torch.autograd.grad(ops.conv_cl(x, wr, s, p, channel_first=cf), wr, dy)
        ref = sum(refs[i][2] for i in items)
        share["dw sparse"] = _show(tag + " dw, dy on the probe items only", R.relerr(dw_s, ref), BAR_DW) / BAR_DW
        assert R.relerr(dw_s, ref) < BAR_DW
    for name, v in share.items():
        print(f"  {tag} {name}: {v:.2f} of its bar")
    torch.cuda.synchronize()
    _peak(dev, need, tag)


@pytest.mark.parametrize("layer,B", R.CONV_2G, ids=[f"{c[0]}-{c[1]}" for c in R.CONV_2G])
def test_conv_2g(layer, B, gpu_device, kernel_log):
    """Forward, input gradient and weight gradient with a tensor just past 2^31 bytes (stated need: CONV_NEED, 12 to 16 GiB).
    The temporal cases run with ``avid_tconv_configure(2)``: every layer that CAN take tconv64 / twgrad64 would."""
    from avid_hip import ops
    if layer.startswith("temporal"):
        assert ops.tconv_configure(2) == 2
    try:
        _conv_case(layer, B, gpu_device, kernel_log)
    finally:
        if layer.startswith("temporal"):
            ops.tconv_configure(-1)


@pytest.mark.parametrize("layer,B", R.CONV_4G, ids=[f"{c[0]}-{c[1]}" for c in R.CONV_4G])
def test_conv_4g(layer, B, gpu_device, kernel_log):
    """The same past 2^32 bytes: a buffer descriptor's num_records no longer fits 32 bits (need: 30 / 20 GiB)."""
    _conv_case(layer, B, gpu_device, kernel_log)


def test_conv_spatial_forward_past_2e31_elements(gpu_device, kernel_log):
    """33 669 000 pixels x 64 channels = 2 154 816 000 elements, 8.6 GB per tensor: forward only (need: 24 GiB)."""
    _conv_case(*R.SPATIAL_2E31, gpu_device, kernel_log, grads=False)


# ================================================================================================================ norm and pool
NORM_NEED = {5400: 16, 10800: 26, 21500: 46}          # GiB: x, y / z, dy / dz, dx (8.6 GB each at B = 21500) + float64 chunks
ROWS = 1 << 20                                        # rows per float64 chunk on the device


def _bn_params(dev):
    g = torch.Generator().manual_seed(41)
    gamma = (torch.rand(64, generator=g) * 3.0 - 1.0).to(dev)                # some negative scales
    beta = (torch.rand(64, generator=g) - 0.5).to(dev)
    rm0, rv0 = torch.randn(64, generator=g).to(dev) * 0.1, (torch.rand(64, generator=g) + 0.5).to(dev)
    return gamma, beta, rm0, rv0


def _stats64(x):
    """mean, biased variance over all rows in float64 on the device (two passes), and what torch's float32 reduction gives."""
    M = x.numel() // 64
    mean = R.sum64(x) / M
    var = R.sum64(x, lambda v: (v - mean) ** 2) / M
    v32, m32 = torch.var_mean(x.reshape(-1, 64), dim=0, unbiased=False)
    return mean, var, m32, v32


def _check_stats(tag, x, s4, rm, rv, rm0, rv0, eps=1e-5, momentum=0.1):
    M = x.numel() // 64
    mean, var, m32, v32 = _stats64(x)
    istd = 1.0 / torch.sqrt(var + eps)
    rm_ref = (1 - momentum) * rm0.double() + momentum * mean
    rv_ref = (1 - momentum) * rv0.double() + momentum * var * M / (M - 1)
    i32 = 1.0 / torch.sqrt(v32.double() + eps)
    out = {}
    for name, got, ref, f32 in (("mean", s4[0], mean, m32), ("invstd", s4[1], istd, i32), ("running_mean", rm, rm_ref, None),
                                ("running_var", rv, rv_ref, None)):
        out[name] = _show(f"{tag} {name}", R.relerr(got, ref), BAR[name], None if f32 is None else R.relerr(f32, ref))
    for name, err in out.items():
        assert err < BAR[name], (tag, name, err)
    return mean, istd


def _bn_rows64(xc, mean, istd, gamma, beta):
    xhat = (xc.double() - mean) * istd
    return xhat, xhat * gamma.double() + beta.double()


def _check_bn_forward(tag, x, y, mean, istd, gamma, beta, relu):
    """The whole y against the float64 formula on the device, in row chunks; returns the worst error over max|ref|."""
    xf, yf = x.reshape(-1, 64), y.reshape(-1, 64)
    worst, scale = 0.0, 0.0
    for o in range(0, xf.shape[0], ROWS):
        _, pre = _bn_rows64(xf[o:o + ROWS], mean, istd, gamma, beta)
        ref = pre.clamp_min(0) if relu else pre
        err = (yf[o:o + ROWS].double() - ref).abs()
        assert not bool(torch.isnan(err).any()), tag
        worst, scale = max(worst, float(err.max())), max(scale, float(ref.abs().max()))
    return worst / scale


def _check_bn_backward(tag, x, dy, pos, dx, dg, db, mean, istd, gamma, beta, relu):
    """dx (whole tensor), dgamma, dbeta against float64 on the device.  ``pos`` (relu): the device's activation, whose sign
    pattern the reference takes — after checking that it disagrees with float64 only where |pre-activation| < 1e-5."""
    xf, dyf, dxf = x.reshape(-1, 64), dy.reshape(-1, 64), dx.reshape(-1, 64)
    pf = pos.reshape(-1, 64) if relu else None
    M = xf.shape[0]
    sdy = torch.zeros(64, dtype=torch.float64, device=x.device)
    sdyx = torch.zeros_like(sdy)
    flips = near = 0
    for o in range(0, M, ROWS):
        xhat, pre = _bn_rows64(xf[o:o + ROWS], mean, istd, gamma, beta)
        d = dyf[o:o + ROWS].double()
        if relu:
            mask = pf[o:o + ROWS] > 0
            f = mask != (pre > 0)
            flips += int(f.sum())
            near += int((pre.abs() < 1e-5).sum())
            assert not bool(f.any()) or float(pre.abs()[f].max()) < 1e-5, (tag, "a ReLU sign differs off a near-tie")
            d = d * mask
        sdy += d.sum(0)
        sdyx += (d * xhat).sum(0)
    assert flips <= near
    worst = scale = 0.0
    k = gamma.double() * istd
    for o in range(0, M, ROWS):
        xhat, _ = _bn_rows64(xf[o:o + ROWS], mean, istd, gamma, beta)
        d = dyf[o:o + ROWS].double()
        if relu:
            d = d * (pf[o:o + ROWS] > 0)
        ref = k * (d - sdy / M - xhat * (sdyx / M))
        err = (dxf[o:o + ROWS].double() - ref).abs()
        assert not bool(torch.isnan(err).any()), tag
        worst, scale = max(worst, float(err.max())), max(scale, float(ref.abs().max()))
    s32 = dyf.sum(0) if not relu else None
    errs = {"dx": _show(f"{tag} dx (whole tensor)", worst / scale, BAR["dx"]),
            "dgamma": _show(f"{tag} dgamma", R.relerr(dg, sdyx), BAR["dgamma"]),
            "dbeta": _show(f"{tag} dbeta", R.relerr(db, sdy), BAR["dbeta"], None if s32 is None else R.relerr(s32, sdy))}
    print(f"  {tag}: ReLU sign flips against float64 {flips}, pre-activations below 1e-5: {near}")
    for name, err in errs.items():
        assert err < BAR[name], (tag, name, err)
    return sdy, sdyx


def _bn_item64(x_i, dy_i, pos_i, mean, istd, gamma, beta, relu, sdy, sdyx, M):
    """One item on the CPU in float64: y and dx by the BatchNorm formulas (the sums over all rows come from the device)."""
    c = lambda t: t.detach().cpu().double()                                   # noqa: E731
    xhat, pre = _bn_rows64(c(x_i), c(mean), c(istd), c(gamma), c(beta))
    y = pre.clamp_min(0) if relu else pre
    d = c(dy_i) * (c(pos_i) > 0) if relu else c(dy_i)
    dx = c(gamma) * c(istd) * (d - c(sdy) / M - xhat * (c(sdyx) / M))
    return y, dx


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("B", R.NORM_B)
def test_batch_norm_train(B, relu, gpu_device):
    """``batch_norm_cl`` forward + backward over [B, 2, 27, 29, 64] (need: NORM_NEED — 16 / 26 / 46 GiB), and ``bn_apply_eval``
    with the saved scale / shift: bit-identical to the training pass's y, whole and in chunks."""
    from avid_hip import ops
    dev = gpu_device
    _need(dev, NORM_NEED[B])
    shape = (B,) + R.NORM_ITEM
    M = B * 2 * 27 * 29
    tag = f"bn{'+relu' if relu else ''} B={B}"
    items = R.probe_items(B, (4 * 2 * 27 * 29 * 64,), seed=1)
    x = R.fill(shape, 31, dev, scale=1.7, shift=0.3)
    dy = R.fill(shape, 32, dev, kind="uniform")
    gamma, beta, rm0, rv0 = _bn_params(dev)
    with guarded(0xFF) as g:
        xr, gr, br = x.detach().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rm, rv = rm0.clone(), rv0.clone()
        cnt = torch.zeros((), dtype=torch.int64, device=dev)
        src = ops.BnSource(None, None, relu)
        y = ops.batch_norm_cl(xr, gr, br, rm, rv, True, 0.1, 1e-5, relu, cnt, src=src)
        dx, dg, db = torch.autograd.grad(y, [xr, gr, br], dy)
        g.check()
        _workspaces_exact(g)
    y, s4 = y.detach(), src.stats4
    src.x = None
    assert int(cnt) == 1
    print()
    R.assert_written(y, tag + " y")
    R.assert_written(dx, tag + " dx")
    # check 3: statistics, running statistics; then the whole y and dx and the backward sums against float64 on the device
    mean, istd = _check_stats(tag, x, s4, rm, rv, rm0, rv0)
    ey = _show(f"{tag} y (whole tensor)", _check_bn_forward(tag, x, y, mean, istd, gamma, beta, relu), BAR["y"])
    assert ey < BAR["y"]
    sdy, sdyx = _check_bn_backward(tag, x, dy, y, dx, dg, db, mean, istd, gamma, beta, relu)
    # check 1: probe items on the CPU
    refs = {i: _bn_item64(x[i], dy[i], y[i], mean, istd, gamma, beta, relu, sdy, sdyx, M) for i in items}
    sy = R.check_probes(y, lambda i: refs[i][0], items, BAR["y"], tag + " y")
    sx = R.check_probes(dx, lambda i: refs[i][1], items, BAR["dx"], tag + " dx")
    print(f"  {tag} probe items {items}: y {sy:.2f}, dx {sx:.2f} of their bars")
    del dx, dy
    # check 2: the apply is per element — the eval-mode apply with the saved scale / shift gives the same bits, whole and chunked
    scale, shift = s4[2].contiguous(), s4[3].contiguous()
    with guarded(0xFF) as g:
        ye = ops.bn_apply_eval(x, scale, shift, relu)
        g.check()
    R.assert_written(ye, tag + " bn_apply_eval")
    assert torch.equal(ye, y), tag + ": bn_apply_eval differs from the training pass's y"
    del ye
    n = R.chunk_items((4 * 2 * 27 * 29 * 64,))
    R.check_chunks(y, lambda b0, b1: ops.bn_apply_eval(x[b0:b1], scale, shift, relu), n, None, tag + " apply")
    torch.cuda.synchronize()
    _peak(dev, NORM_NEED[B], tag)


def _pool_item(x_i):
    """ATen on the CPU, float32 (max is exact): y and the gradient routing of one item [T, H, W, C]."""
    xr = x_i.detach().cpu().permute(3, 0, 1, 2).unsqueeze(0).clone().requires_grad_(True)
    return xr, F.max_pool3d(xr, (1, 3, 3), (1, 2, 2), (0, 1, 1))


@pytest.mark.parametrize("B", R.NORM_B)
def test_maxpool_hw3s2(B, gpu_device):
    """``maxpool_hw3s2`` forward + backward on post-ReLU data (many exact ties at 0) over [B, 2, 27, 29, 64] -> [B, 2, 14, 15, 64];
    need: 12 / 22 / 40 GiB."""
    from avid_hip import ops
    dev = gpu_device
    need = {5400: 12, 10800: 22, 21500: 40}[B]
    _need(dev, need)
    tag = f"maxpool B={B}"
    ib = (4 * 2 * 27 * 29 * 64, 4 * 2 * 14 * 15 * 64)
    items = R.probe_items(B, ib, seed=1)
    x = R.fill((B,) + R.NORM_ITEM, 51, dev).clamp_min_(0)
    dy = R.fill((B, 2, 14, 15, 64), 52, dev, kind="uniform")
    with guarded(0xFF) as g:
        xr = x.detach().requires_grad_(True)
        y = ops.maxpool_hw3s2(xr)
        (dx,) = torch.autograd.grad(y, xr, dy)
        g.check()
    y = y.detach()
    R.assert_written(y, tag + " y")
    R.assert_written(dx, tag + " dx")
    for i in items:                                    # check 1: bit-equal values, ATen's routing incl. ties
        xr, yr = _pool_item(x[i])
        (yr * dy[i].cpu().permute(3, 0, 1, 2).unsqueeze(0)).sum().backward()
        assert torch.equal(y[i].cpu().permute(3, 0, 1, 2), yr.detach()[0]), (tag, i)
        torch.testing.assert_close(dx[i].cpu().permute(3, 0, 1, 2), xr.grad[0], rtol=1e-6, atol=1e-7, msg=f"{tag} dx item {i}")
    n = R.chunk_items(ib)                              # check 2: the same bits as on chunks below 1 GiB
    chunk_dx = {}

    def run_chunk(b0, b1):
        xc = x[b0:b1].detach().requires_grad_(True)
        yc = ops.maxpool_hw3s2(xc)
        (chunk_dx[b0],) = torch.autograd.grad(yc, xc, dy[b0:b1])
        return yc.detach()

    R.check_chunks(y, run_chunk, n, None, tag + " y")
    R.check_chunks(dx, lambda b0, b1: chunk_dx.pop(b0), n, None, tag + " dx")
    torch.cuda.synchronize()
    _peak(dev, need, tag)


@pytest.mark.parametrize("B", R.NORM_B)
def test_bn_relu_maxpool(B, gpu_device):
    """The video stem's tail, ``bn_relu_maxpool`` forward + backward and its eval form (need: NORM_NEED): statistics and running
    statistics against float64; the pooled output bit-equal to ``maxpool_hw3s2(bn_apply_eval(x, scale, shift, relu))`` and to
    ``bn_relu_maxpool_eval`` (whole and chunked) — the same fma and a max; dx / dgamma / dbeta against the float64 BatchNorm
    backward of the gradient ``maxpool_hw3s2`` routes (pinned by the test above)."""
    from avid_hip import ops
    dev = gpu_device
    _need(dev, NORM_NEED[B])
    tag = f"bn_relu_maxpool B={B}"
    M = B * 2 * 27 * 29
    ib = (4 * 2 * 27 * 29 * 64, 4 * 2 * 14 * 15 * 64)
    items = R.probe_items(B, ib, seed=1)
    x = R.fill((B,) + R.NORM_ITEM, 61, dev, scale=1.7, shift=0.3)
    dyp = R.fill((B, 2, 14, 15, 64), 62, dev, kind="uniform")
    gamma, beta, rm0, rv0 = _bn_params(dev)
    with guarded(0xFF) as g:
        xr, gr, br = x.detach().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rm, rv = rm0.clone(), rv0.clone()
        cnt = torch.zeros((), dtype=torch.int64, device=dev)
        y = ops.bn_relu_maxpool(xr, gr, br, rm, rv, 0.1, 1e-5, cnt)
        s4 = y.grad_fn.saved_tensors[2]
        dx, dg, db = torch.autograd.grad(y, [xr, gr, br], dyp)
        g.check()
        _workspaces_exact(g)
    y = y.detach()
    assert int(cnt) == 1 and s4.shape == (4, 64)
    print()
    R.assert_written(y, tag + " y")
    R.assert_written(dx, tag + " dx")
    mean, istd = _check_stats(tag, x, s4, rm, rv, rm0, rv0)
    scale, shift = s4[2].contiguous(), s4[3].contiguous()
    # eval form, whole and chunked: the same bits
    with guarded(0xFF) as g:
        ye = ops.bn_relu_maxpool_eval(x, scale, shift)
        g.check()
    R.assert_written(ye, tag + " eval")
    assert torch.equal(ye, y), tag + ": the eval form differs from the training pass's pooled output"
    del ye
    n = R.chunk_items(ib)
    R.check_chunks(y, lambda b0, b1: ops.bn_relu_maxpool_eval(x[b0:b1], scale, shift), n, None, tag + " eval")
    # the separate ops on the same saved map
    z = ops.bn_apply_eval(x, scale, shift, True).requires_grad_(True)
    p = ops.maxpool_hw3s2(z)
    assert torch.equal(p.detach(), y), tag + ": pooled output differs from maxpool_hw3s2(bn_apply_eval(x))"
    (dz,) = torch.autograd.grad(p, z, dyp)
    del p
    z = z.detach()
    # check 1: pooled probe items against float64 on the CPU (max of the float64 activations)
    c = lambda t: t.detach().cpu().double()                                   # noqa: E731

    def y_ref(i):
        _, pre = _bn_rows64(c(x[i]), c(mean), c(istd), c(gamma), c(beta))
        return F.max_pool3d(pre.clamp_min(0).permute(3, 0, 1, 2).unsqueeze(0), (1, 3, 3), (1, 2, 2), (0, 1, 1))[0].permute(1, 2, 3, 0)

    sy = R.check_probes(y, y_ref, items, BAR["y"], tag + " y")
    print(f"  {tag} probe items {items}: y {sy:.2f} of its bar")
    sdy, sdyx = _check_bn_backward(tag, x, dz, z, dx, dg, db, mean, istd, gamma, beta, True)
    refs = {i: _bn_item64(x[i], dz[i], z[i], mean, istd, gamma, beta, True, sdy, sdyx, M) for i in items}
    sx = R.check_probes(dx, lambda i: refs[i][1], items, BAR["dx"], tag + " dx")
    print(f"  {tag} dx probe items: {sx:.2f} of the bar")
    torch.cuda.synchronize()
    _peak(dev, NORM_NEED[B], tag)


@pytest.mark.parametrize("B", R.NORM_B)
def test_relu_bwd_and_colsum(B, gpu_device):
    """``avid_relu_bwd`` over B x 100224 elements (past 2^31 at B = 21500) and ``avid_colsum`` over B x 1566 rows of 64, through
    ``lib.call`` (need: 10 / 18 / 34 GiB)."""
    from avid_hip import lib, ops
    dev = gpu_device
    need = {5400: 10, 10800: 18, 21500: 34}[B]
    _need(dev, need)
    tag = f"relu_bwd/colsum B={B}"
    shape = (B,) + R.NORM_ITEM
    items = R.probe_items(B, (4 * 2 * 27 * 29 * 64,), seed=1)
    y = R.fill(shape, 71, dev)
    dy = R.fill(shape, 72, dev, kind="uniform")
    with guarded(0xFF) as g:
        dx = torch.empty(shape, dtype=torch.float32, device=dev)
        out = torch.empty(64, dtype=torch.float32, device=dev)
        lib.call("avid_relu_bwd", y.numel(), ops._p(y), ops._p(dy), ops._p(dx), ops._stream())
        lib.call("avid_colsum", y.numel() // 64, 64, ops._p(dy), ops._p(out), ops._stream())
        g.check()
    R.assert_written(dx, tag + " dx")
    R.assert_written(out, tag + " colsum")
    R.check_probes(dx, lambda i: torch.where(y[i] > 0, dy[i], torch.zeros_like(dy[i])).cpu().double(), items, 0.0, tag)
    n = R.chunk_items((4 * 2 * 27 * 29 * 64,))

    def run_chunk(b0, b1):
        o = torch.full_like(dy[b0:b1], float("nan"))
        lib.call("avid_relu_bwd", o.numel(), ops._p(y[b0:b1]), ops._p(dy[b0:b1]), ops._p(o), ops._stream())
        return o

    R.check_chunks(dx, run_chunk, n, None, tag)
    ref = R.sum64(dy)
    print()
    err = _show(tag + " colsum", R.relerr(out, ref), BAR["colsum"], R.relerr(dy.reshape(-1, 64).sum(0), ref))
    assert err < BAR["colsum"]
    torch.cuda.synchronize()
    _peak(dev, need, tag)
