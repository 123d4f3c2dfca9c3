"""Every launch of the benchmark's batch-64 step that is not a convolution, against float64, at its own shape and with the
step's own arguments — and the step's Adam launches.

The table (tests/golden/bs64_norm_ops.json, checked against the launch programs by tests/test_bs64_table.py) lists each
distinct BatchNorm, stem BatchNorm + max-pool, global max-pool, ReLU-backward and column-sum record, and the flat Adam buffer
with its split.  Each case calls the same C entry point with the same arguments csrc/program.hip passes, every output filled
with NaN first and the running statistics started away from 0 / 1:
  * bn_fwd: x is the real output of its producing convolution (tests/test_gpu_bs64_layers._fwd), fed post-ReLU data
    (``randn`` for the stems, as bench.py feeds them), so the partial rows are the producer's own, in its count and layout.
    mean, invstd, scale, shift, y and the running statistics against float64 BatchNorm of the device's own x;
    num_batches_tracked + 1.  A statistics-only entry (y = NULL) is bit-identical to the same launch with y.
  * bn_bwd: dy is the consumer's input gradient with the fused BatchNorm-backward sums (or the global pool's gradient
    where the record has no partial rows), the saved state that of the matching forward.
  * the stem's BatchNorm + ReLU + max-pool, at full size with the stem convolution's own partial rows.
  * global max-pool, ReLU backward and column sums with ties; Adam over the bench's flat length and split.
Reference: tests/_f64conv.bn_ref (float64, proven against F.batch_norm by tests/test_bs64_table.py), built on the device.

Bars (test_gpu_ops.test_batchnorm_train's, none loosened): max|err| / max|ref| below 1e-5 for y, 1e-6 running_mean, 1e-5
running_var, 2e-5 dx / dgamma / dbeta; mean 1e-6 and invstd 1e-5.  ``pytest -s`` prints every error next to its bar, and
each forward's max |mean| * invstd (how far the layer's activations sit from zero)."""
import pytest
import torch

import _f64conv as R
import test_gpu_bs64_layers as CL

pytestmark = pytest.mark.gpu

TABLE = R.load_bs64_norm_table()
OPS = TABLE["ops"]
BAR = {"mean": 1e-6, "invstd": 1e-5, "scale": 1e-5, "shift": 1e-5, "y": 1e-5, "running_mean": 1e-6, "running_var": 1e-5,
       "dx": 2e-5, "dgamma": 2e-5, "dbeta": 2e-5, "colsum": 1e-6}
NBT0 = 17                    # num_batches_tracked before the launch
# the kernels of the records this file runs (csrc/norm_pool.hip, csrc/optim.hip): the coverage test counts their launches
NORM_KERNELS = ("bn_", "global_maxpool_", "relu_bwd_kernel", "colsum_kernel", "adam_flat_kernel")


def relerr(a, b):
    a, b = a.double(), b.double().to(a.device)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _check(tag, name, got, want, bar):
    err = relerr(got, want)
    print(f"  {tag:32s} {name:14s} max {err:.2e} / {bar:.0e}")
    assert bool(torch.isfinite(got).all()), (tag, name, "an element was never written")
    assert err < bar, (tag, name, err)


def _ws(dev, M, C_):
    from avid_hip import lib, ops
    return ops.workspace(dev, lib.raw("avid_bn_workspace_bytes")(M, C_))


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _bn_params(C_, dev, seed):
    """gamma (some negative), beta, and running statistics away from their initial 0 / 1."""
    g = CL._gen(dev, seed)
    gamma = torch.randn(C_, generator=g, device=dev) * 0.5 + 1.0
    beta = torch.randn(C_, generator=g, device=dev) * 0.2
    rm = torch.randn(C_, generator=g, device=dev) * 0.3
    rv = torch.rand(C_, generator=g, device=dev) * 2.0 + 0.5
    return gamma, beta, rm, rv


def _produce(prod, dev, seed):
    """The producing convolution's output [M, C] and its BatchNorm partial rows, from the data the step feeds it: the stems
    read randn clips, every other layer the output of a BatchNorm + ReLU (the in-affine form: that map applied on the fly)."""
    from avid_hip import ops
    e = CL.LAYERS[prod["conv"]]
    form = prod["fwd"]
    x, w, _ = CL._inputs(e, dev, seed)
    addend = None
    if form[0]:
        osz = tuple(R.out_size(n, kk, s, p) for n, kk, s, p in zip(e["x"][1:], e["k"], e["stride"], e["pad"]))
        addend = torch.randn((e["x"][0],) + osz + (e["Cout"],), generator=CL._gen(dev, seed + 1), device=dev).clamp_min_(0)
    if form[4]:
        xd = x.double().reshape(-1, e["Cin"])
        invstd = (1.0 / xd.std(0, unbiased=False)).float().contiguous()
        shift = (-xd.mean(0).float() * invstd).contiguous()
        y, part = ops.conv_fwd_in(x, w, tuple(e["stride"]), tuple(e["pad"]), invstd, shift, relu=form[4] == 2,
                                  addend=addend, bn_stats=True)
    else:
        if not e["channel_first"]:
            x.clamp_min_(0)
        y, part = CL._fwd(e, x, w, form, addend=addend)
    return y.reshape(-1, e["Cout"]), part


def _bn_fwd(e, x, part, gamma, beta, rm, rv, with_y=True):
    """avid_bn_fwd_train as csrc/program.hip calls it (AVID_OP_BN_FWD); returns y (or None), the saved [4][C] and the counter."""
    from avid_hip import lib, ops
    M, C_ = e["M"], e["C"]
    dev = x.device
    y = _nan((M, C_), dev) if with_y else None
    s4 = _nan((4, C_), dev)
    nbt = torch.full((), NBT0, dtype=torch.int64, device=dev)
    ws = _ws(dev, M, C_)
    lib.call("avid_bn_fwd_train", M, C_, ops._p(x), ops._p(gamma), ops._p(beta), ops._p(rm), ops._p(rv), float(e["momentum"]),
             float(e["eps"]), e["relu"], ops._p(y), ops._p(s4[0]), ops._p(s4[1]), ops._p(s4[2]), ops._p(s4[3]), ops._p(nbt),
             ops._p(part), e["nparts"], ops._p(ws), ws.numel(), ops._stream())
    return y, s4, nbt


def _bn_bwd(e, x, dy, gamma, s4, part):
    from avid_hip import lib, ops
    M, C_ = e["M"], e["C"]
    dev = x.device
    dx, dgamma, dbeta = _nan((M, C_), dev), _nan((C_,), dev), _nan((C_,), dev)
    ws = _ws(dev, M, C_)
    lib.call("avid_bn_bwd", M, C_, ops._p(x), ops._p(dy), ops._p(gamma), ops._p(s4[0]), ops._p(s4[1]), ops._p(s4[2]),
             ops._p(s4[3]), e["relu"], ops._p(dx), ops._p(dgamma), ops._p(dbeta), ops._p(part), e["nparts"], e["frozen"],
             ops._p(ws), ws.numel(), ops._stream())
    return dx, dgamma, dbeta


def _fma_mask(x, s4):
    """The ReLU's pass pattern as the kernels decide it: fma(x, scale, shift) > 0 in float32 (exact through float64)."""
    return (x.double() * s4[2].double() + s4[3].double()).float() > 0


def _check_fwd(name, e, x, y, s4, nbt, rm0, rv0, rm, rv, gamma, beta):
    ref = R.bn_ref(x, gamma, beta, rm0, rv0, e["momentum"], e["eps"], relu=bool(e["relu"]),
                   mask=_fma_mask(x, s4) if e["relu"] else None)
    ratio = float((ref["mean"].abs() * ref["invstd"]).max())
    print(f"  {'max |mean| * invstd':32s} {name:14s} {ratio:.3f}   ({e['nparts']} partial rows, M {e['M']})")
    for k, got in (("mean", s4[0]), ("invstd", s4[1]), ("scale", s4[2]), ("shift", s4[3]), ("running_mean", rm),
                   ("running_var", rv)):
        _check(k, name, got, ref[k], BAR[k])
    if y is not None:
        _check("y", name, y, ref["y"], BAR["y"])
    assert int(nbt) == NBT0 + 1, int(nbt)
    return ref


def _forward_case(fi, dev):
    """Run bn_fwd entry fi on its producer's output: (entry, x, partial rows, params, y, s4, nbt, running stats, their start)."""
    e = OPS["bn_fwd"][fi]
    x, part = _produce(e["producer"], dev, 4000 + 10 * fi)
    assert part.shape[0] == e["nparts"], (part.shape, e["nparts"])
    gamma, beta, rm0, rv0 = _bn_params(e["C"], dev, 5000 + fi)
    rm, rv = rm0.clone(), rv0.clone()
    y, s4, nbt = _bn_fwd(e, x, part, gamma, beta, rm, rv, with_y=e["y"])
    return e, x, part, (gamma, beta), y, s4, nbt, (rm, rv), (rm0, rv0)


@pytest.mark.parametrize("fi", range(len(OPS["bn_fwd"])), ids=[R.norm_id("bn_fwd", e) for e in OPS["bn_fwd"]])
def test_bn_fwd_against_float64(fi, gpu_device):
    dev = gpu_device
    e, x, part, (gamma, beta), y, s4, nbt, (rm, rv), (rm0, rv0) = _forward_case(fi, dev)
    name = f"fwd{fi}"
    print(f"\n{R.norm_id('bn_fwd', e)}: producer {e['producer']}, y {e['y']}")
    _check_fwd(name, e, x, y, s4, nbt, rm0, rv0, rm, rv, gamma, beta)
    if not e["y"]:
        # statistics only: the saved vectors and running statistics are those of the same launch writing y
        rm2, rv2 = rm0.clone(), rv0.clone()
        y2, s42, nbt2 = _bn_fwd(e, x, part, gamma, beta, rm2, rv2, with_y=True)
        assert torch.equal(s42, s4) and torch.equal(rm2, rm) and torch.equal(rv2, rv) and int(nbt2) == int(nbt)
        assert bool(torch.isfinite(y2).all())


def _consumer_dy(e, x_in, s4, dev, seed):
    """dy of a BatchNorm backward as the step makes it: the consumer's input gradient with the fused BatchNorm-backward sums
    (csrc/program.hip AVID_OP_CONV_DGRAD, i[4] = 1), reading this BatchNorm's input and saved state."""
    from avid_hip import lib, ops
    prod = e["producer"]
    ce = CL.LAYERS[prod["conv"]]
    form = prod["dgrad"]
    _, w, dyc = CL._inputs(ce, dev, seed)
    g = CL._gen(dev, seed + 1)
    addend = add_stride = None
    if form[1]:
        if any(form[2:]):
            add_stride = tuple(form[2:])
            cshape = (ce["x"][0],) + tuple(-(-n // s) for n, s in zip(ce["x"][1:], add_stride)) + (ce["Cin"],)
            addend = torch.randn(cshape, generator=g, device=dev)
        else:
            addend = torch.randn(tuple(ce["x"]) + (ce["Cin"],), generator=g, device=dev)
    rows = CL._desc(ce)[0].bn_bwd_rows
    assert rows == e["nparts"], (rows, e["nparts"])
    part = _nan((rows, 2, ce["Cin"]), dev)
    fuse = lib.BnBwdFuse(ops._p(x_in), ops._p(s4[2]), ops._p(s4[3]), ops._p(s4[0]), ops._p(s4[1]), e["relu"], ops._p(part))
    dy = CL._dgrad(ce, dyc, w, addend=addend, add_stride=add_stride, fuse=fuse)
    return dy.reshape(-1, ce["Cin"]), part


def _gpool_dy(e, y, dev, seed):
    """dy from the global max-pool's backward over this BatchNorm's output (the last layer of a tower)."""
    from avid_hip import lib, ops
    C_ = e["C"]
    pool = [p for p in OPS["gpool_bwd"] if p["C"] == C_ and p["B"] * p["S"] == e["M"]]
    assert len(pool) == 1
    B, S = pool[0]["B"], pool[0]["S"]
    yp, am = _nan((B, C_), dev), torch.full((B, C_), -1, dtype=torch.int32, device=dev)
    lib.call("avid_global_maxpool_fwd", B, S, C_, ops._p(y), ops._p(yp), ops._p(am), ops._stream())
    dyp = torch.randn((B, C_), generator=CL._gen(dev, seed), device=dev)
    dy = _nan((e["M"], C_), dev)
    lib.call("avid_global_maxpool_bwd", B, S, C_, ops._p(dyp), ops._p(am), ops._p(dy), ops._stream())
    return dy


@pytest.mark.parametrize("bi", range(len(OPS["bn_bwd"])), ids=[R.norm_id("bn_bwd", e) for e in OPS["bn_bwd"]])
def test_bn_bwd_against_float64(bi, gpu_device):
    dev = gpu_device
    e = OPS["bn_bwd"][bi]
    fe, x, _, (gamma, beta), y, s4, _, _, _ = _forward_case(e["fwd"], dev)
    assert (fe["M"], fe["C"], fe["relu"]) == (e["M"], e["C"], e["relu"])
    print(f"\n{R.norm_id('bn_bwd', e)}: forward {R.norm_id('bn_fwd', fe)}, producer {e['producer']}")
    if e["producer"] is not None:
        dy, part = _consumer_dy(e, x.reshape(tuple(CL.LAYERS[e["producer"]["conv"]]["x"]) + (e["C"],)), s4, dev, 6000 + bi)
    else:
        assert e["dy"] == "gpool_bwd" and e["nparts"] == 0 and y is not None
        dy, part = _gpool_dy(e, y, dev, 6000 + bi), None
    dx, dgamma, dbeta = _bn_bwd(e, x, dy, gamma, s4, part)
    ref = R.bn_ref(x, gamma, beta, gamma, gamma, relu=bool(e["relu"]), dy=dy,
                   mask=_fma_mask(x, s4) if e["relu"] else None)
    name = f"bwd{bi}"
    _check("dx", name, dx, ref["dx"], BAR["dx"])
    _check("dgamma", name, dgamma, ref["dgamma"], BAR["dgamma"])
    _check("dbeta", name, dbeta, ref["dbeta"], BAR["dbeta"])


def _window_views(t, fill):
    """The 9 (dh, dw) taps of the stem pool's (1,3,3) / stride (1,2,2) / pad (0,1,1) windows over t [B,T,H,W,C], scan order."""
    B, T, H, W, C_ = t.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tp = torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1), value=fill)
    return [tp[:, :, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2, :] for dh in range(3) for dw in range(3)], tp


def test_stem_bn_pool_against_float64(gpu_device):
    """The video stem's BatchNorm + ReLU + max-pool (avid_bn_relu_maxpool_fwd / _bwd) at 64 x 8 x 56 x 56 x 64 with the stem
    convolution's own partial rows: each pooled value is its window's maximum of the device's normalised values and its
    argmax the first one; saved state, running statistics, dx, dgamma and dbeta against float64."""
    from avid_hip import lib, ops
    dev = gpu_device
    (fe,), (be,) = OPS["bn_pool_fwd"], OPS["bn_pool_bwd"]
    B, T, H, W, C_ = fe["B"], fe["T"], fe["H"], fe["W"], fe["C"]
    assert (B, T, H, W, C_) == (be["B"], be["T"], be["H"], be["W"], be["C"])
    x, part = _produce(fe["producer"], dev, 7000)
    assert part.shape[0] == fe["nparts"]
    M = B * T * H * W
    gamma, beta, rm0, rv0 = _bn_params(C_, dev, 7001)
    rm, rv = rm0.clone(), rv0.clone()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    yp = _nan((B, T, Ho, Wo, C_), dev)
    am = torch.full((B, T, Ho, Wo, C_), 255, dtype=torch.uint8, device=dev)
    s4 = _nan((4, C_), dev)
    nbt = torch.full((), NBT0, dtype=torch.int64, device=dev)
    ws = _ws(dev, M, C_)
    lib.call("avid_bn_relu_maxpool_fwd", B, T, H, W, C_, ops._p(x), ops._p(gamma), ops._p(beta), ops._p(rm), ops._p(rv),
             float(fe["momentum"]), float(fe["eps"]), ops._p(yp), ops._p(am), ops._p(s4[0]), ops._p(s4[1]), ops._p(s4[2]),
             ops._p(s4[3]), ops._p(nbt), ops._p(part), fe["nparts"], ops._p(ws), ws.numel(), ops._stream())
    print("\nstem bn_pool: producer", fe["producer"])
    ref = _check_fwd("stem", dict(fe, M=M, relu=1), x, None, s4, nbt, rm0, rv0, rm, rv, gamma, beta)
    del ref
    # pooling: the device's own normalised values (fma, then ReLU), window maxima, first-maximum argmax
    z = (x.double() * s4[2].double() + s4[3].double()).float().clamp_min_(0).reshape(B, T, H, W, C_)
    taps, _ = _window_views(z, float("-inf"))
    best = taps[0].clone()
    slot = torch.zeros(best.shape, dtype=torch.uint8, device=dev)
    for k in range(1, 9):
        better = taps[k] > best
        best = torch.where(better, taps[k], best)
        slot[better] = k
    del taps
    assert torch.equal(yp, best), "a pooled value is not its window's maximum"
    assert torch.equal(am, slot), "an argmax is not the window's first maximum"
    print(f"  pooled values / argmax exact; {float((best == 0).double().mean()):.3f} of the windows are all zero")
    del best, slot
    # backward: pooled dy routed to the argmax positions, then BatchNorm + ReLU backward
    dyp = torch.randn((B, T, Ho, Wo, C_), generator=CL._gen(dev, 7002), device=dev)
    dx, dgamma, dbeta = _nan((B, T, H, W, C_), dev), _nan((C_,), dev), _nan((C_,), dev)
    lib.call("avid_bn_relu_maxpool_bwd", B, T, H, W, C_, ops._p(x), ops._p(dyp), ops._p(am), ops._p(gamma), ops._p(s4[0]),
             ops._p(s4[1]), ops._p(s4[2]), ops._p(s4[3]), ops._p(dx), ops._p(dgamma), ops._p(dbeta), ops._p(ws), ws.numel(),
             ops._stream())
    dyu = torch.zeros((B, T, H + 2, W + 2, C_), dtype=torch.float64, device=dev)
    dypd = dyp.double()
    for k in range(9):
        dh, dw = divmod(k, 3)
        dyu[:, :, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2, :] += torch.where(am == k, dypd, torch.zeros_like(dypd))
    dyu = dyu[:, :, 1:H + 1, 1:W + 1, :].reshape(M, C_)
    del dypd
    ref = R.bn_ref(x, gamma, beta, rm0, rv0, relu=True, dy=dyu, mask=_fma_mask(x, s4))
    _check("dx", "stem", dx.reshape(M, C_), ref["dx"], BAR["dx"])
    _check("dgamma", "stem", dgamma, ref["dgamma"], BAR["dgamma"])
    _check("dbeta", "stem", dbeta, ref["dbeta"], BAR["dbeta"])


@pytest.mark.parametrize("pi", range(len(OPS["gpool_fwd"])), ids=[R.norm_id("gpool_fwd", e) for e in OPS["gpool_fwd"]])
def test_gpool_exact(pi, gpu_device):
    """Global max-pool over [B, S, C] post-ReLU data (zeros tie; one all-zero column): values exact, argmax the first
    maximum, the backward routes each pooled gradient to that position alone."""
    from avid_hip import lib, ops
    dev = gpu_device
    e = OPS["gpool_fwd"][pi]
    assert {"B": e["B"], "S": e["S"], "C": e["C"], "count": 1} in OPS["gpool_bwd"]
    B, S, C_ = e["B"], e["S"], e["C"]
    x = torch.randn((B, S, C_), generator=CL._gen(dev, 8000 + pi), device=dev).clamp_min_(0)
    x[3, :, 7] = 0.0                                    # an all-zero window: the first position
    x[5, 2, 9] = x[5, 4, 9] = x[5, :, 9].max() + 1.0    # an exact tie between two positions: the first
    y, am = _nan((B, C_), dev), torch.full((B, C_), -1, dtype=torch.int32, device=dev)
    lib.call("avid_global_maxpool_fwd", B, S, C_, ops._p(x), ops._p(y), ops._p(am), ops._stream())
    want_y, want_am = x.max(1)
    first = (x == want_y[:, None, :]).int().argmax(1)   # the first position holding the maximum
    assert torch.equal(y, want_y) and torch.equal(am.long(), first.long())
    assert int(am[3, 7]) == 0 and int(am[5, 9]) == 2
    dyp = torch.randn((B, C_), generator=CL._gen(dev, 8100 + pi), device=dev)
    dx = _nan((B, S, C_), dev)
    lib.call("avid_global_maxpool_bwd", B, S, C_, ops._p(dyp), ops._p(am), ops._p(dx), ops._stream())
    want = torch.zeros_like(x).scatter_(1, first[:, None, :].long(), dyp[:, None, :])
    assert torch.equal(dx, want)


@pytest.mark.parametrize("ri", range(len(OPS["relu_bwd"])), ids=[R.norm_id("relu_bwd", e) for e in OPS["relu_bwd"]])
def test_relu_bwd_exact(ri, gpu_device):
    from avid_hip import lib, ops
    dev = gpu_device
    n = OPS["relu_bwd"][ri]["n"]
    y = torch.randn(n, generator=CL._gen(dev, 8200), device=dev).clamp_min_(0)
    y[:6] = torch.tensor([0.0, -0.0, 2e-38, 0.0, 3.0, 0.0], device=dev)      # zeros of both signs, the smallest normals
    dy = torch.randn(n, generator=CL._gen(dev, 8201), device=dev)
    dx = _nan((n,), dev)
    lib.call("avid_relu_bwd", n, ops._p(y), ops._p(dy), ops._p(dx), ops._stream())
    assert torch.equal(dx, torch.where(y > 0, dy, torch.zeros_like(dy)))


@pytest.mark.parametrize("ci", range(len(OPS["colsum"])), ids=[R.norm_id("colsum", e) for e in OPS["colsum"]])
def test_colsum_against_float64(ci, gpu_device):
    from avid_hip import lib, ops
    dev = gpu_device
    M, C_ = OPS["colsum"][ci]["M"], OPS["colsum"][ci]["C"]
    x = torch.randn((M, C_), generator=CL._gen(dev, 8300 + ci), device=dev) * 3.0 + 0.5
    x[:, 0] = 0.0
    out = _nan((C_,), dev)
    lib.call("avid_colsum", M, C_, ops._p(x), ops._p(out), ops._stream())
    _check("colsum", f"{M}x{C_}", out, x.double().sum(0), BAR["colsum"])


# ---- Adam -----------------------------------------------------------------------------------------------------------
# avid_adam_flat takes its hyper-parameters as float32 (include/avid_hip.h): the float64 reference and the float32 torch
# yardstick both run with the values the kernel receives.  (beta2 = 0.999 arrives as 0.99900001287: an optimizer with that
# beta2, whose moments differ from those of an exact 0.999 by up to 1.3e-5 — a property of the interface, not an error of
# the arithmetic measured here.)
LR, B1, B2, EPS, WD = (float(torch.tensor(h, dtype=torch.float32)) for h in (2e-4, 0.9, 0.999, 1e-8, 1e-5))


def _adam_ref(p, g, m, v, t, lr, grad_scale):
    """One float64 step of torch.optim.Adam (L2 weight decay folded into the gradient, bias-corrected), in place."""
    gg = g.double() * grad_scale + WD * p
    m.mul_(B1).add_((1 - B1) * gg)
    v.mul_(B2).add_((1 - B2) * gg * gg)
    denom = v.sqrt() / (1 - B2 ** t) ** 0.5 + EPS
    p.sub_(lr / (1 - B1 ** t) * m / denom)


def _grads(n, dev, seed):
    """Gradients by index class: 0 exact zeros, 1 ~1e-20 (eps-dominated), 2 ~1e-3, 3 ~1e4."""
    g = torch.randn(n, generator=CL._gen(dev, seed), device=dev)
    cls = torch.arange(n, device=dev) % 4
    scale = torch.tensor([0.0, 1e-20, 1e-3, 1e4], device=dev)[cls]
    return g * scale, cls


def _class_errors(got, ref, cls):
    return [relerr(got[cls == c], ref[cls == c]) for c in range(4)]


@pytest.mark.parametrize("grad_scale", [1.0, 0.5], ids=["scale1", "scale_half"])
def test_adam_bench_split_against_float64(grad_scale, gpu_device):
    """The step's Adam as parallel.TrainStep._optimizer_step_overlapped issues it: the flat buffer's exact length, two launches
    split at adam_early, the second with advance=False, step_dev and lr_dev set, weight decay 1e-5.  Five steps, then the
    counter set to 10^4 and one more.  p, m and v against float64 Adam, per gradient class (zeros, 1e-20, 1e-3, 1e4): no worse
    than 2x what torch.optim.Adam(foreach=False) makes in float32 of the same data."""
    from avid_hip import ops
    dev = gpu_device
    n, early = TABLE["adam"]["n"], TABLE["adam"]["early"]
    p = torch.randn(n, generator=CL._gen(dev, 9000), device=dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    t_dev = torch.zeros((), dtype=torch.int64, device=dev)
    lr_dev = torch.full((), LR, dtype=torch.float32, device=dev)
    pr, mr, vr = p.double(), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, foreach=False)
    for k, t in enumerate([1, 2, 3, 4, 5, 10001]):
        if t == 10001:
            t_dev.fill_(10000)
            opt.state[pt]["step"].fill_(10000)
        g, cls = _grads(n, dev, 9100 + k)
        kw = dict(grad_scale=grad_scale, step_dev=t_dev, lr_dev=lr_dev)
        ops.adam_flat(p[:early], g[:early], m[:early], v[:early], 0.5, B1, B2, EPS, WD, 0, **kw)   # (host lr: ignored)
        ops.adam_flat(p[early:], g[early:], m[early:], v[early:], 0.5, B1, B2, EPS, WD, 0, advance=False, **kw)
        _adam_ref(pr, g, mr, vr, t, LR, grad_scale)
        pt.grad = g * grad_scale                          # (exact: a power of two)
        opt.step()
    torch.cuda.synchronize()
    assert int(t_dev) == 10001
    st = opt.state[pt]
    print(f"\nadam n={n} split {early}, grad_scale {grad_scale}: per class [0, 1e-20, 1e-3, 1e4]")
    for tag, got, torch32, ref in (("p", p, pt.detach(), pr), ("m", m, st["exp_avg"], mr), ("v", v, st["exp_avg_sq"], vr)):
        assert bool(torch.isfinite(got).all()), tag
        e_dev, e_t = _class_errors(got, ref, cls), _class_errors(torch32, ref, cls)
        print(f"  {tag}: kernel {['%.2e' % e for e in e_dev]}  torch fp32 {['%.2e' % e for e in e_t]}")
        for c in range(4):
            assert e_dev[c] <= 2 * e_t[c], (tag, c, e_dev[c], e_t[c])


@pytest.mark.parametrize("n", [4097, 4098, 4099, 100003])
def test_adam_tail_against_float64(n, gpu_device):
    """n % 4 = 1, 2, 3 (the tail block-0 handles): every element against float64, NaN sentinels past the end untouched."""
    from avid_hip import ops
    dev = gpu_device
    pad = 8
    bufs = [torch.full((n + pad,), float("nan"), device=dev) for _ in range(4)]
    p, g, m, v = (b[:n] for b in bufs)
    p.copy_(torch.randn(n, generator=CL._gen(dev, 9200), device=dev))
    m.zero_()
    v.zero_()
    pr, mr, vr = p.double(), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    for t in range(1, 4):
        g.copy_(_grads(n, dev, 9300 + t)[0])
        ops.adam_flat(p, g, m, v, LR, B1, B2, EPS, WD, t)
        _adam_ref(pr, g, mr, vr, t, LR, 1.0)
    for b in (bufs[0], bufs[2], bufs[3]):
        assert bool(torch.isnan(b[n:]).all()), "Adam wrote past the end of its buffer"
    for tag, got, ref in (("p", p, pr), ("m", m, mr), ("v", v, vr)):
        err = relerr(got, ref)
        tail = relerr(got[n - n % 4:], ref[n - n % 4:]) if n % 4 else 0.0
        print(f"  adam n={n} {tag}: max {err:.2e}, tail {tail:.2e} / 1e-06")
        assert err < 1e-6 and tail < 1e-6, (tag, err, tail)


@pytest.mark.parametrize("host_lr", [0.0, 1e-3])
def test_adam_lr_dev_without_step_dev(host_lr, gpu_device):
    """include/avid_hip.h: with lr_dev set the learning rate is read from it instead of ``lr`` — also when the step comes by
    value (step_dev NULL) and the host's lr is 0 (the first value of a warm-up schedule)."""
    from avid_hip import ops
    dev = gpu_device
    n = 100003
    p = torch.randn(n, generator=CL._gen(dev, 9400), device=dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    lr_dev = torch.full((), LR, dtype=torch.float32, device=dev)
    pr, mr, vr = p.double(), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    p0 = p.clone()
    for t in range(1, 4):
        g = _grads(n, dev, 9500 + t)[0]
        ops.adam_flat(p, g, m, v, host_lr, B1, B2, EPS, WD, t, lr_dev=lr_dev)
        _adam_ref(pr, g, mr, vr, t, LR, 1.0)
    moved = pr - p0.double()
    err = float((p.double() - p0.double() - moved).abs().max() / moved.abs().max())
    print(f"\n  adam lr_dev, host lr {host_lr}: update error {err:.2e} / 1e-2, p {relerr(p, pr):.2e} / 1e-06")
    assert err < 1e-2, err                       # (the update is ~1e-3 of p: p's own rounding is ~1e-3 of it)
    assert relerr(p, pr) < 1e-6


# ---- coverage -------------------------------------------------------------------------------------------------------
def _norm_names(report):
    return {k: v["launches"] for k, v in report.items() if k.startswith(NORM_KERNELS)}


def test_table_covers_the_steps_other_kernels(gpu_device, kernel_log):
    """One default batch-64 engine step (bench.py's configuration) launches exactly the BatchNorm / pool / ReLU-backward /
    column-sum kernels the table implies: each entry's launch, run here with its own arguments, times its record count.  (Under
    the launch log the engine issues its Adam update as one launch over the whole buffer: parallel.TrainStep.step.)"""
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
    eng.step(video, audio, ids)
    with kernel_log() as log:
        eng.step(video, audio, ids)
    step = _norm_names(log.report)
    del eng, model, crit, video, audio
    torch.cuda.empty_cache()

    want = {}

    def logged(count, fn):
        with kernel_log() as lg:
            fn()
        for k, nl in _norm_names(lg.report).items():
            want[k] = want.get(k, 0) + count * nl

    for e in OPS["bn_fwd"]:
        M, C_ = e["M"], e["C"]
        x, part = torch.randn(M, C_, device=dev), torch.rand(max(e["nparts"], 1), 2, C_, device=dev) + 1.0
        gamma, beta, rm, rv = _bn_params(C_, dev, 1)
        logged(e["count"], lambda: _bn_fwd(e, x, part if e["nparts"] else None, gamma, beta, rm, rv, with_y=e["y"]))
    for e in OPS["bn_bwd"]:
        M, C_ = e["M"], e["C"]
        x, dy, part = torch.randn(M, C_, device=dev), torch.randn(M, C_, device=dev), torch.rand(max(e["nparts"], 1), 2, C_, device=dev)
        s4 = torch.rand(4, C_, device=dev) + 0.5
        logged(e["count"], lambda: _bn_bwd(e, x, dy, s4[2], s4, part if e["nparts"] else None))
    for fe, be in zip(OPS["bn_pool_fwd"], OPS["bn_pool_bwd"]):
        B, T, H, W, C_ = fe["B"], fe["T"], fe["H"], fe["W"], fe["C"]
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x, part = torch.randn(B, T, H, W, C_, device=dev), torch.rand(fe["nparts"], 2, C_, device=dev) + 1.0
        gamma, beta, rm, rv = _bn_params(C_, dev, 1)
        yp, am = torch.empty(B, T, Ho, Wo, C_, device=dev), torch.zeros(B, T, Ho, Wo, C_, dtype=torch.uint8, device=dev)
        s4 = torch.empty(4, C_, device=dev)
        ws = _ws(dev, B * T * H * W, C_)
        logged(fe["count"], lambda: lib.call(
            "avid_bn_relu_maxpool_fwd", B, T, H, W, C_, ops._p(x), ops._p(gamma), ops._p(beta), ops._p(rm), ops._p(rv), 0.1,
            1e-5, ops._p(yp), ops._p(am), ops._p(s4[0]), ops._p(s4[1]), ops._p(s4[2]), ops._p(s4[3]), None, ops._p(part),
            fe["nparts"], ops._p(ws), ws.numel(), ops._stream()))
        dx, dg, db = torch.empty_like(x), torch.empty(C_, device=dev), torch.empty(C_, device=dev)
        logged(be["count"], lambda: lib.call(
            "avid_bn_relu_maxpool_bwd", B, T, H, W, C_, ops._p(x), ops._p(yp), ops._p(am), ops._p(gamma), ops._p(s4[0]),
            ops._p(s4[1]), ops._p(s4[2]), ops._p(s4[3]), ops._p(dx), ops._p(dg), ops._p(db), ops._p(ws), ws.numel(),
            ops._stream()))
        del x, yp, am, dx
    for kind in ("gpool_fwd", "gpool_bwd"):
        for e in OPS[kind]:
            B, S, C_ = e["B"], e["S"], e["C"]
            x, y, am = torch.randn(B, S, C_, device=dev), torch.empty(B, C_, device=dev), torch.zeros(B, C_, dtype=torch.int32, device=dev)
            if kind == "gpool_fwd":
                logged(e["count"], lambda: lib.call("avid_global_maxpool_fwd", B, S, C_, ops._p(x), ops._p(y), ops._p(am), ops._stream()))
            else:
                logged(e["count"], lambda: lib.call("avid_global_maxpool_bwd", B, S, C_, ops._p(y), ops._p(am), ops._p(x), ops._stream()))
    for e in OPS["relu_bwd"]:
        a, b, c = (torch.randn(e["n"], device=dev) for _ in range(3))
        logged(e["count"], lambda: lib.call("avid_relu_bwd", e["n"], ops._p(a), ops._p(b), ops._p(c), ops._stream()))
    for e in OPS["colsum"]:
        a, o = torch.randn(e["M"], e["C"], device=dev), torch.empty(e["C"], device=dev)
        logged(e["count"], lambda: lib.call("avid_colsum", e["M"], e["C"], ops._p(a), ops._p(o), ops._stream()))
    want["adam_flat_kernel"] = 1
    print("\nstep:", sorted(step.items()), "\ntable:", sorted(want.items()))
    assert step.get("adam_flat_kernel") == 1
    assert step == want
