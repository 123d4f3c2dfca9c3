"""Every convolution of the benchmark's batch-64 step against float64, at its own shape and under the default dispatch.

The layer table (tests/golden/bs64_conv_layers.json, checked against the model by tests/test_bs64_table.py) lists each
distinct geometry of the step's launch programs and what the step fuses into it.  For each entry, through the same C entry
points and arguments ``ops.conv_cl`` / ``ops.conv_fwd_in`` / ``ops.conv_wgrad_in`` issue, with every output filled with NaN
first (an element no kernel writes fails):
  * forward, with each epilogue form the step uses (residual addend, BatchNorm partial sums, bias / ReLU); the partial sums
    against float64 column sums of the device's own output over all rows;
  * input gradient, with each form the step uses (BatchNorm-backward sums of the producer, dense or compact strided addend);
  * weight gradient on its own, and the step's grouped weight-gradient launches with the step's own groups.
Reference: tests/_f64conv.py (im2col + float64 matmul, proven against F.conv3d by tests/test_bs64_table.py).

Bars (those of tests/test_gpu_ops.py / test_gpu_precision.py, none loosened): max|err| / max|ref| below 2e-5 for outputs and
input gradients, 5e-5 for weight gradients; BatchNorm partial sums within 1e-5 of the largest column's sum of |terms|;
rms(err) / rms(ref) <= 6e-7 for every direction whose product kernels (reduce kernels aside) all belong to the
six-bf16-product families of test_gpu_precision.CASES — except the three long weight-gradient contractions of LONG_WGRAD,
see there.  ``pytest -s`` prints the measured error of every geometry and direction next to its bar.

Which kernels serve each direction is pinned per entry (tests/golden/bs64_conv_kernels.json, recorded on an MI355X under the
default dispatch): a silent dispatch change fails here, and test_layer_table_covers_the_steps_convolution_kernels keeps the
table complete against a real step.

The checks themselves (check_layer, check_in_affine, check_group) take the table entry and the pinned kernels as arguments:
tests/test_gpu_ft_layers.py runs the fine-tuning programs' tables through the same code."""
import json
import os
import ctypes as C

import pytest
import torch

import _f64conv as R

pytestmark = pytest.mark.gpu

TABLE = R.load_bs64_table()
LAYERS = TABLE["layers"]
with open(os.path.join(R.HERE, "golden", "bs64_conv_kernels.json")) as _f:
    KERNELS = json.load(_f)
N_GEOMETRIES = 32
CONV_FAMILIES = ("igemm_pk_kernel", "wino", "tconv64", "twgrad64", "stem_", "wgrad_", "splitk_reduce")
# (stem_fwd3_kernel: the video stem's forward where the pre-split patch of stem_fwd3p_kernel does not fit — the 224 x 224 clips
# of tests/test_gpu_ft_layers.py; the same six products)
SIX_PRODUCT = ("igemm_pk_kernel", "stem_fwd3_kernel", "stem_fwd3p_kernel", "stem_wgrad3_kernel", "tconv64_kernel",
               "twgrad64_kernel", "wino2p_kernel", "wgrad_tab_kernel")
# kernels that only add up slabs a product kernel wrote (no products of their own): left out when the family is decided
REDUCE = ("splitk_reduce", "wgrad_reduce", "wgrad_group_reduce", "stem_wgrad_reduce")
# Weight gradients whose rms error against float64 is above RMS_BAR because the contraction itself is long — RMS_BAR was set
# on test_gpu_precision's shapes (contractions of at most ~60 k rows).  For these the bar is the precision test's other one:
# within 3x of a plain float32 contraction of the same data (tests/_f64conv.py, dtype=float32).  Measured on an MI355X,
# rms(err)/rms(ref) of the kernel, then of float32:
#   video stem, stem_wgrad3_kernel, 1.6 M rows:                              4.8e-6 vs 4.0e-6 (1.2x)
#   conv2x temporal, twgrad64_kernel, 401 k rows: plain form                 9.9e-7 vs 2.4e-6 (0.41x)
#                                                 in-affine, ReLU / linear    8.4e-7 vs 1.7e-6 (0.50x), 9.8e-7 vs 2.4e-6 (0.41x)
#   conv3x.0 strided spatial, wgrad_tab_kernel<2,2>, 100 k rows:              6.9e-7 vs 2.0e-6 (0.35x)
# (only the stem is less accurate than float32 itself).  Every other direction of the table meets RMS_BAR.
LONG_WGRAD = ("3to64_k377_s122_x8x112x112_cf", "64to64_k311_s111_x8x28x28", "64to128_k133_s122_x8x28x28")
BAR = {"y": 2e-5, "dx": 2e-5, "dw": 5e-5}
RMS_BAR = 6e-7


def relerr(a, b):
    a, b = a.double(), b.double().to(a.device)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rms_rel(a, b):
    a, b = a.double(), b.double().to(a.device)
    return float(((a - b) ** 2).mean().sqrt() / ((b ** 2).mean().sqrt() + 1e-300))


def conv_names(report):
    """The convolution-family kernels of a launch log (the Winograd weight transform is a weight-table kernel, not one)."""
    return sorted(k for k in report if any(k.startswith(f) for f in CONV_FAMILIES) and not k.startswith("wino_weight"))


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _inputs(e, dev, seed):
    """x (channels-last, or [B,C,T,H,W] for a stem), weight (library layout) and dy of a table entry."""
    from avid_hip import ops
    g = _gen(dev, seed)
    B, Ti, Hi, Wi = e["x"]
    cin, cout, k = e["Cin"], e["Cout"], tuple(e["k"])
    shape = (B, cin, Ti, Hi, Wi) if e["channel_first"] else (B, Ti, Hi, Wi, cin)
    x = torch.randn(shape, generator=g, device=dev)
    w = ops.make_weight(cout, cin, *k).to(dev)
    w.copy_(torch.randn((cout, cin) + k, generator=g, device=dev) * (cin * k[0] * k[1] * k[2]) ** -0.5)
    osz = tuple(R.out_size(n, kk, s, p) for n, kk, s, p in zip((Ti, Hi, Wi), k, e["stride"], e["pad"]))
    dy = torch.randn((B,) + osz + (cout,), generator=g, device=dev)
    return x, w, dy


def _desc(e):
    from avid_hip import ops
    return ops._desc_cached(tuple(e["x"]), e["Cin"], e["Cout"], tuple(e["k"]), tuple(e["stride"]), tuple(e["pad"]),
                            e["channel_first"])


def _ws(dev, nb):
    from avid_hip import ops
    return ops.workspace(dev, nb) if nb else None


def _fwd(e, x, w, form, addend=None, bias=None):
    """avid_conv_fwd as ops._ConvCL.forward calls it, y and partials pre-filled with NaN."""
    from avid_hip import lib, ops
    d, nb, _, _, srows = _desc(e)
    has_add, want_stats, has_bias, relu, _ = form
    y = torch.full((d.B, d.To, d.Ho, d.Wo, d.Cout), float("nan"), device=x.device)
    stats = None
    if want_stats:
        assert srows > 0, "the step takes BatchNorm partial sums from this layer, the library offers none"
        stats = torch.full((srows, 2, d.Cout), float("nan"), device=x.device)
    ws = _ws(x.device, nb)
    plain = bias is None and not relu
    lib.call("avid_conv_fwd", C.byref(d), ops._p(x), ops._p(w), ops._p(ops._fwd_u(w, d, plain)),
             ops._p(addend if has_add else None), ops._p(bias if has_bias else None), int(relu), ops._p(y), ops._p(stats),
             ops._p(ws), ws.numel() if ws is not None else 0, ops._stream())
    return y, stats


def _dgrad(e, dy, w, addend=None, add_stride=None, fuse=None):
    from avid_hip import lib, ops
    d, _, nbd, _, _ = _desc(e)
    dx = torch.full((d.B, d.Ti, d.Hi, d.Wi, d.Cin), float("nan"), device=dy.device)
    ws = _ws(dy.device, nbd)
    lib.call("avid_conv_dgrad", C.byref(d), ops._p(dy), ops._p(w), ops._p(ops._wt_for(w)), ops._p(ops._dgrad_u(w, d)),
             ops._p(addend), (C.c_int32 * 3)(*add_stride) if add_stride is not None else None, ops._p(dx),
             C.byref(fuse) if fuse is not None else None, ops._p(ws), ws.numel() if ws is not None else 0, ops._stream())
    return dx


def _wgrad(e, x, dy, w):
    from avid_hip import lib, ops
    d, _, _, nbw, _ = _desc(e)
    dw = torch.full_like(w, float("nan"))
    ws = _ws(x.device, nbw)
    lib.call("avid_conv_wgrad", C.byref(d), ops._p(x), ops._p(dy), ops._p(dw), ops._p(ws), ws.numel() if ws is not None else 0,
             ops._stream())
    return dw


def _bn_producer(e, dev, seed):
    """Synthetic saved state of a training-mode BatchNorm(+ReLU) whose output is this layer's input: its input xb, and
    mean / invstd / scale / shift with some negative scales (avid_bn_fwd_train's four vectors)."""
    g = _gen(dev, seed)
    B, Ti, Hi, Wi = e["x"]
    c = e["Cin"]
    xb = torch.randn((B, Ti, Hi, Wi, c), generator=g, device=dev) * 1.7 + 0.3
    mean = torch.randn(c, generator=g, device=dev) * 0.2 + 0.3
    invstd = torch.rand(c, generator=g, device=dev) * 0.6 + 0.5
    gamma = torch.rand(c, generator=g, device=dev) * 3.0 - 1.0
    beta = torch.rand(c, generator=g, device=dev) - 0.5
    scale = (gamma * invstd).contiguous()
    shift = (beta - mean * scale).contiguous()
    return xb, mean, invstd, scale, shift


def _check(tag, name, got, want, bar, kernels, results, fp32=None):
    """max|err| / max|ref| below ``bar``; rms bar as in the module docstring.  ``fp32``: a callable giving the same contraction
    in plain float32 — passed for the weight gradients of LONG_WGRAD only, which are held to 3x of it instead of RMS_BAR."""
    err = relerr(got, want)
    rms = rms_rel(got, want)
    products = [k for k in kernels if not k.startswith(REDUCE)]
    six = bool(products) and all(k.startswith(SIX_PRODUCT) for k in products)
    print(f"  {tag:28s} {name:12s} max {err:.2e} / {bar:.0e}   rms {rms:.2e}{' / %.0e' % RMS_BAR if six else ''}   {kernels}")
    results.append((tag, name, err, rms))
    assert bool(torch.isfinite(got).all()), (tag, name, "an element was never written")
    assert err < bar, (tag, name, err)
    if six and fp32 is not None:
        rms32 = rms_rel(fp32(), want)
        print(f"  {'':28s} {name:12s} rms {rms:.2e}: float32 contraction {rms32:.2e}, ratio {rms / rms32:.2f} / 3")
        assert rms <= 3 * rms32, (tag, name, rms, rms32)
    elif six:
        assert rms <= RMS_BAR, (tag, name, rms)


def _expect_kernels(pins, name, key, ks):
    """The kernels that served one direction are the ones pinned for it (``pins``: a table's pinned-kernels file)."""
    want = pins["layers"][name][key] if name is not None else key
    assert ks == want, (name, key, ks, want)


def _form_key(direction, form):
    return direction + " " + ",".join(map(str, form))


def _check_sums(tag, name, got, terms, results):
    """got [rows][Cout] partial rows of a column sum of ``terms`` [M][Cout] (float64): their total within 1e-5 of the largest
    column's sum of |terms| (test_gpu_ops.test_conv_bn_partials's bar, written without the division)."""
    assert bool(torch.isfinite(got).all()), (tag, name, "a partial row was never written")
    tot = got.double().sum(0)
    ref = terms.sum(0)
    err = float((tot - ref).abs().max() / terms.abs().sum(0).max())
    print(f"  {tag:28s} {name:12s} max {err:.2e} / 1e-05")
    results.append((tag, name, err, None))
    assert err < 1e-5, (tag, name, err)


@pytest.fixture(autouse=True)
def _default_dispatch(gpu_device):
    """The default dispatch is what runs: every switch at its environment / default value."""
    from avid_hip import lib, ops
    lib.raw("avid_tconv_configure")(-1)
    ops.wino_configure()
    ops.wino2_configure()
    yield


def test_table_has_every_geometry():
    assert len(LAYERS) == N_GEOMETRIES
    assert all(e["fwd"] or e["dgrad"] for e in LAYERS)


def check_layer(e, idx, pins, dev, kernel_log, long_wgrad=(), chunk=8):
    """One table entry in every form the programs use, against float64 and the pinned kernels (the module docstring's
    checks).  ``long_wgrad``: the ids whose weight gradient is held to 3x float32 (LONG_WGRAD's rule); ``chunk``: clips per
    slice of the float64 reference."""
    from avid_hip import ops
    name = R.layer_id(e)
    d = _desc(e)[0]
    x, w, dy = _inputs(e, dev, 1000 + idx)
    x_cl = x.permute(0, 2, 3, 4, 1) if e["channel_first"] else x
    want = tuple(n for n, use in (("y", e["fwd"]), ("dx", e["dgrad"]), ("dw", e["wgrad"])) if use)
    ref = R.conv_ref(x_cl, w, tuple(e["stride"]), tuple(e["pad"]), dy=dy, want=want, chunk=chunk)
    res = []
    print(f"\n{name}: fwd {e['fwd']} dgrad {e['dgrad']} wgrad {e['wgrad']}")
    g = _gen(dev, 2000 + idx)
    for form in e["fwd"]:
        if form[4]:
            continue          # (the in-affine form: test_conv2x_temporal_layer_in_the_programs_form)
        addend = torch.randn_like(ref["y"], dtype=torch.float32) if form[0] else None
        bias = torch.randn(e["Cout"], generator=g, device=dev) if form[2] else None
        with kernel_log() as log:
            y, stats = _fwd(e, x, w, form, addend=addend, bias=bias)
        ks = conv_names(log.report)
        want_y = ref["y"] + (addend.double() if addend is not None else 0) + (bias.double() if bias is not None else 0)
        if form[3]:
            want_y = want_y.clamp_min(0)
        _check(f"fwd{form}", name, y, want_y, BAR["y"], ks, res)
        if stats is not None:
            yd = y.double().reshape(-1, e["Cout"])
            _check_sums("fwd bn sums", name, stats[:, 0], yd, res)
            _check_sums("fwd bn squares", name, stats[:, 1], yd * yd, res)
        _expect_kernels(pins, name, _form_key("fwd", form), ks)
    for form in e["dgrad"]:
        bn_sums, has_add = form[:2]
        strided = any(form[2:])
        addend = add_stride = fuse = None
        want_dx = ref["dx"].clone()
        if has_add:
            if strided:
                add_stride = tuple(form[2:])
                Ti, Hi, Wi = e["x"][1:]
                cshape = (e["x"][0],) + tuple(-(-n // s) for n, s in zip((Ti, Hi, Wi), add_stride)) + (e["Cin"],)
                addend = torch.randn(cshape, generator=g, device=dev)
                want_dx[:, ::add_stride[0], ::add_stride[1], ::add_stride[2], :] += addend.double()
            else:
                addend = torch.randn(tuple(x.shape), generator=g, device=dev)
                want_dx += addend.double()
        if bn_sums:
            from avid_hip import lib
            assert d.bn_bwd_rows > 0, "the step fuses BatchNorm-backward sums into this layer, the library offers none"
            xb, mean, invstd, scale, shift = _bn_producer(e, dev, 3000 + idx)
            part = torch.full((d.bn_bwd_rows, 2, e["Cin"]), float("nan"), device=dev)
            fuse = lib.BnBwdFuse(ops._p(xb), ops._p(scale), ops._p(shift), ops._p(mean), ops._p(invstd), 1, ops._p(part))
        with kernel_log() as log:
            dx = _dgrad(e, dy, w, addend=addend, add_stride=add_stride, fuse=fuse)
        ks = conv_names(log.report)
        _check(f"dgrad{form}", name, dx, want_dx, BAR["dx"], ks, res)
        _expect_kernels(pins, name, _form_key("dgrad", form), ks)
        if bn_sums:
            # sum dy_m and sum dy_m * xhat over all rows, dy_m = the device's own dx masked by the producer's ReLU: the sign of
            # fma(x, scale, shift), which float64 gives exactly (a float32 multiply-then-add rounds twice and flips about one
            # element in 25 million, a whole term of the sum)
            xbd = xb.double().reshape(-1, e["Cin"])
            mask = ((xbd * scale.double() + shift.double()) > 0).double()
            dym = dx.double().reshape(-1, e["Cin"]) * mask
            xhat = (xbd - mean.double()) * invstd.double()
            _check_sums("dgrad bn-bwd sum dy", name, part[:, 0], dym, res)
            _check_sums("dgrad bn-bwd sum dy*xhat", name, part[:, 1], dym * xhat, res)
    if "dw" in want:
        with kernel_log() as log:
            dw = _wgrad(e, x, dy, w)
        ks = conv_names(log.report)
        fp32 = None
        if name in long_wgrad:
            fp32 = lambda: R.conv_ref(x_cl, w, tuple(e["stride"]), tuple(e["pad"]), dy=dy, want=("dw",),  # noqa: E731
                                      chunk=chunk, dtype=torch.float32)["dw"]
        _check("wgrad", name, dw, ref["dw"], BAR["dw"], ks, res, fp32=fp32)
        _expect_kernels(pins, name, "wgrad", ks)
    return res


@pytest.mark.parametrize("idx", range(len(LAYERS)), ids=[R.layer_id(e) for e in LAYERS])
def test_layer_against_float64(idx, gpu_device, kernel_log):
    check_layer(LAYERS[idx], idx, KERNELS, gpu_device, kernel_log, long_wgrad=LONG_WGRAD)


def _conv2x_temporal(layers=LAYERS):
    es = [e for e in layers if any(f[4] for f in e["fwd"])]
    assert len(es) == 1
    return es[0]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_conv2x_temporal_layer_in_the_programs_form(relu, gpu_device, kernel_log):
    """conv2x's temporal layer as the launch programs run it at 64 clips (avid_conv_fwd_in / avid_conv_wgrad_in: the
    BatchNorm (+ReLU) in front applied while staging): against float64 of conv(relu(x * scale + shift)) with negative scales,
    with and without the residual addend, BatchNorm partial sums included; bit-identical to the same layer reading the
    normalised tensor; tconv64_kernel / twgrad64_kernel under the default dispatch; the in-affine launch counter moves."""
    e = _conv2x_temporal()
    assert e["x"] == [64, 8, 28, 28] and e["Cin"] == e["Cout"] == 64 and e["wgrad"] == ["in_affine"]
    assert R.layer_id(e) in LONG_WGRAD
    check_in_affine(e, relu, KERNELS, gpu_device, kernel_log, long_wgrad=LONG_WGRAD)


def check_in_affine(e, relu, pins, dev, kernel_log, long_wgrad=(), chunk=8):
    """A 64-channel temporal layer in the in-affine forms of the programs (the checks of
    test_conv2x_temporal_layer_in_the_programs_form), against float64 and the pinned kernels."""
    from avid_hip import lib, ops
    name = R.layer_id(e)
    assert e["Cin"] == e["Cout"] == 64
    stride, pad = tuple(e["stride"]), tuple(e["pad"])
    x, w, dy = _inputs(e, dev, 77)
    xb = _bn_producer(e, dev, 78)[0]
    # the normalised tensor as avid_bn_fwd_train writes it (fma(x, scale, shift) (+ max(., 0))) and the scale / shift it saved
    gamma = (torch.rand(64, generator=_gen(dev, 80), device=dev) * 3.0 - 1.0).contiguous()          # some negative scales
    beta = (torch.rand(64, generator=_gen(dev, 81), device=dev) - 0.5).contiguous()
    src = ops.BnSource(None, None, relu)
    z = ops.batch_norm_cl(xb, gamma, beta, torch.zeros(64, device=dev), torch.ones(64, device=dev), True, relu=relu, src=src)
    scale, shift = src.stats4[2].contiguous(), src.stats4[3].contiguous()
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    zd = xb.double() * scale.double() + shift.double()
    if relu:
        zd = zd.clamp_min(0)
    ref = R.conv_ref(zd, w, stride, pad, dy=dy, want=("y", "dw"), chunk=chunk)
    count = lib.raw("avid_debug_in_affine_launches")
    add = torch.randn(tuple(ref["y"].shape), generator=_gen(dev, 79), device=dev)
    res = []
    print(f"\n{name} (in-affine, relu={relu})")
    for addend in (None, add):
        form = [int(addend is not None), 1, 0, 0, 0]
        y_ref, p_ref = _fwd(e, z, w, form, addend=addend)
        before = count(1), count(0)
        with kernel_log() as log:
            y, part = ops.conv_fwd_in(xb, w, stride, pad, scale, shift, relu=relu, addend=addend, bn_stats=True)
        assert (count(1) - before[0], count(0) - before[1]) == (1, 0)
        ks = conv_names(log.report)
        assert log.launches("tconv64_kernel<0>") == 1
        _expect_kernels(pins, None, pins["in_affine"]["fwd"], ks)
        assert torch.equal(y, y_ref) and torch.equal(part, p_ref)
        want_y = ref["y"] + (addend.double() if addend is not None else 0)
        _check(f"fwd_in add={addend is not None}", name, y, want_y, BAR["y"], ks, res)
        yd = y.double().reshape(-1, 64)
        _check_sums("fwd_in bn sums", name, part[:, 0], yd, res)
        _check_sums("fwd_in bn squares", name, part[:, 1], yd * yd, res)
    plain = _wgrad(e, z, dy, w)
    before = count(1)
    with kernel_log() as log:
        dw = ops.conv_wgrad_in(xb, dy, w, stride, pad, scale, shift, relu=relu)
    assert count(1) - before == 1
    ks = conv_names(log.report)
    _expect_kernels(pins, None, pins["in_affine"]["wgrad"], ks)
    assert torch.equal(dw, plain)
    fp32 = None
    if name in long_wgrad:
        fp32 = lambda: R.conv_ref(z, w, stride, pad, dy=dy, want=("dw",), chunk=chunk, dtype=torch.float32)["dw"]  # noqa: E731
    _check("wgrad_in", name, dw, ref["dw"], BAR["dw"], ks, res, fp32=fp32)
    return res


def _group_items(members, dev, seed, layers=LAYERS):
    from avid_hip import lib, ops
    items = (lib.WgradItem * len(members))()
    keep, outs = [], []
    for j, i in enumerate(members):
        e = layers[i]
        x, w, dy = _inputs(e, dev, seed + 17 * j + i)
        d = _desc(e)[0]
        assert d.groupable, R.layer_id(e)
        dw = torch.full_like(w, float("nan"))
        items[j].d = d
        items[j].x, items[j].dy, items[j].dw = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
        keep.append((e, x, w, dy))
        outs.append(dw)
    nb = lib.raw("avid_conv_wgrad_group_workspace_bytes")(len(members), items)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)
    return items, keep, outs, ws


def _run_group(items, n, ws):
    from avid_hip import lib, ops
    lib.call("avid_conv_wgrad_group", n, items, ops._p(ws), ws.numel(), ops._stream())


@pytest.mark.parametrize("gi", range(len(TABLE["groups"])), ids=[f"group{i}" for i in range(len(TABLE["groups"]))])
def test_grouped_weight_gradients_of_the_step(gi, gpu_device, kernel_log):
    """Each grouped weight-gradient launch of the batch-64 backward program (avid_conv_wgrad_group), with the step's own
    items in the step's order, every item against float64 (5e-5 of its scale)."""
    check_group(TABLE, gi, KERNELS, gpu_device, kernel_log)


def check_group(table, gi, pins, dev, kernel_log, chunk=8):
    """Grouped weight-gradient launch ``gi`` of a table with the programs' own items, every item against float64."""
    layers, members = table["layers"], table["groups"][gi]
    items, keep, outs, ws = _group_items(members, dev, 500 * gi, layers)
    with kernel_log() as log:
        _run_group(items, len(members), ws)
    ks = conv_names(log.report)
    _expect_kernels(pins, None, pins["groups"][gi], ks)
    print(f"\ngroup {gi}: {[R.layer_id(layers[i]) for i in members]}")
    res = []
    for (e, x, w, dy), dw in zip(keep, outs):
        ref = R.conv_ref(x, w, tuple(e["stride"]), tuple(e["pad"]), dy=dy, want=("dw",), chunk=chunk)
        _check("grouped wgrad", R.layer_id(e), dw, ref["dw"], BAR["dw"], ks, res)
    return res


def test_layer_table_covers_the_steps_convolution_kernels(gpu_device, kernel_log):
    """One default batch-64 engine step (bench.py's configuration) launches no convolution-family kernel that the layer
    table's runs (every entry in every form, the grouped launches, the in-affine forms) did not launch as well."""
    import criterions
    import models
    from avid_hip import lib, ops
    from avid_hip.parallel import TrainStep
    dev = gpu_device
    torch.manual_seed(0)
    model = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).to(dev).train()
    crit = criterions.AVID(num_data=240000, embedding_dim=128, num_negatives=1024, momentum=0.5, device=dev.index)
    eng = TrainStep(model, crit, lr=2e-4, weight_decay=1e-5)
    g = torch.Generator().manual_seed(1234)
    video = torch.randn(*R.BENCH_VIDEO, generator=g).to(dev)
    audio = torch.randn(*R.BENCH_AUDIO, generator=g).to(dev)
    ids = torch.randperm(240000, generator=torch.Generator().manual_seed(99))[:64].to(dev)
    eng.step(video, audio, ids)                    # (compiles the programs, builds the weight tables)
    with kernel_log() as log:
        eng.step(video, audio, ids)
    step_kernels = set(conv_names(log.report))
    del eng, model, crit, video, audio
    torch.cuda.empty_cache()

    ran = set()
    for idx, e in enumerate(LAYERS):
        x, w, dy = _inputs(e, dev, 1000 + idx)
        with kernel_log() as log:
            for form in e["fwd"]:
                if form[4]:
                    c = e["Cin"]
                    sc, sh = torch.ones(c, device=dev), torch.zeros(c, device=dev)
                    ops.conv_fwd_in(x, w, tuple(e["stride"]), tuple(e["pad"]), sc, sh, relu=True,
                                    addend=torch.zeros_like(dy) if form[0] else None, bn_stats=bool(form[1]))
                else:
                    _fwd(e, x, w, form, addend=torch.zeros_like(dy) if form[0] else None,
                         bias=torch.zeros(e["Cout"], device=dev) if form[2] else None)
            for form in e["dgrad"]:
                bn_sums, has_add = form[:2]
                strided = any(form[2:])
                addend = add_stride = fuse = None
                if has_add:
                    add_stride = tuple(form[2:]) if strided else None
                    shp = tuple(x.shape) if not strided else (e["x"][0],) + tuple(
                        -(-n // s) for n, s in zip(e["x"][1:], add_stride)) + (e["Cin"],)
                    addend = torch.zeros(shp, device=dev)
                if bn_sums:
                    xb, mean, invstd, scale, shift = _bn_producer(e, dev, 1)
                    part = torch.empty((_desc(e)[0].bn_bwd_rows, 2, e["Cin"]), device=dev)
                    fuse = lib.BnBwdFuse(ops._p(xb), ops._p(scale), ops._p(shift), ops._p(mean), ops._p(invstd), 1,
                                         ops._p(part))
                _dgrad(e, dy, w, addend=addend, add_stride=add_stride, fuse=fuse)
            if "own" in e["wgrad"]:
                _wgrad(e, x, dy, w)
            if "in_affine" in e["wgrad"]:
                c = e["Cin"]
                ops.conv_wgrad_in(x, dy, w, tuple(e["stride"]), tuple(e["pad"]), torch.ones(c, device=dev),
                                  torch.zeros(c, device=dev), relu=True)
        ran |= set(conv_names(log.report))
    for gi, members in enumerate(TABLE["groups"]):
        items, keep, outs, ws = _group_items(members, dev, 500 * gi)
        with kernel_log() as log:
            _run_group(items, len(members), ws)
        ran |= set(conv_names(log.report))
    print("\nstep:", sorted(step_kernels), "\nlayer runs:", sorted(ran))
    assert step_kernels, "the step's launch log holds no convolution kernel"
    missing = sorted(step_kernels - ran)
    assert not missing, missing
