"""The persistent kernels against float64 under reduced CU budgets (``ops.set_cu_budget`` / ``AVID_CU_RESERVE``).

Every persistent kernel sizes its grid and deals its work from the CU count it plans for.  At the small tensors of the
per-kernel tests and all 256 CUs the planner only produces tails without whole rounds; under a budget of 8-40 CUs the mixed
plans (whole rounds + an unsplit or K-split tail + the reduce over rows >= tail_row0, rot != 0, the weight-stationary order,
three column blocks on an unpaired grid, a compact grid, a single tail unit) appear at 600-7000 rows, where a float64
reference costs a second.  The rows are tests/_budget_ref.py's table, which tests/test_cu_budget_host.py pins on the host
and holds to cover every class; here each row runs forward, input gradient and weight gradient under its budget:

* the plan the library reports under the budget is the table's, and the launch log shows that family (and the reduce);
* the error bars are the project's existing ones: max-error relative to the scale below 2e-5 / 2e-5 / 5e-5 for y / dx / dw
  (tests/test_gpu_ops.py), and for the six-product kernels rms error against float64 <= 6e-7 of rms(output) and <= 3x
  the float32 host run's (tests/test_gpu_precision.py);
* a second call under the same budget gives the same bits;
* where the budget's plan and the full-budget plan are both unsplit on the same kernel template, y and dx are the
  full-budget run's bits (a whole tile has the same contraction order wherever it is dealt);
* the BatchNorm-statistics epilogue (write_stats' owner column block, pk_rot, pk_ws) and the BatchNorm-backward sums out of
  the input gradient hold test_conv_bn_partials' / test_bn_backward_partials_from_dgrad's assertions under the budget.

The Winograd kernels, the stems and the grouped weight gradient follow with their own tests' bars at budgets 8 and 24.
Every test restores the budget; a budget at or above the device's CU count is skipped, and on a 256-CU device none is.

Worst figures measured on a 256-CU MI355X (the `[budget]` lines), against the bar of each column:

  table rows        max error / scale     y 1.16e-06 (s128@24)   dx 1.32e-06 (s128@24)   dw 1.97e-06 (wino256@8)   bars 2e-5 / 2e-5 / 5e-5
  six-product       rms error / rms       y 4.84e-07 (s128@24)   dx 4.82e-07 (s128@24)   dw 3.17e-07 (t64@8)       bar 6e-7
  kernels           x float32 host run    y 2.48 (t256@16)       dx 2.46 (t256@16)       dw 1.21 (t64@8)           bar 3
  partial rows      column sums 3.16e-07, sums of squares 1.41e-07 (wino256@8)                                     bar 1e-5
  conv-BN-conv chain, gradients with the hand-over against without: 3.12e-07 (chain64@8)                           bar 2e-5
  Winograd test     y 5.12e-07, dx 4.77e-07, dw 3.33e-06 (128 channels, wino_kernel, 8 CUs)                        bars 2e-5 / 2e-5 / 5e-5
  stems             y 3.29e-07, dw 1.12e-06 (video, 8 CUs)                                                         bars 2e-5 / 5e-5
  grouped weight gradients   2.29e-06 (8 CUs)                                                                      bar 5e-5

A whole tile under a small budget accumulates its full contraction in one fp32 chain where the full-budget plan of the same
layer sums f short K pieces: the rms error of y / dx is 1.5-2.5 times the full-budget run's (s64: 1.47e-07 at 256 CUs, 3.52e-07
at 8; s128, K = 1152: 3.53e-07 and 4.84e-07), still inside both bars.  Likewise the fp32 weight gradients whose pixel chunks
grow as the grid shrinks (wino_wgrad_kernel at 256 channels: max error 4.0e-07 at 256 CUs, 1.97e-06 at 8).
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import _budget_ref as R
from oracle import detgen
from test_gpu_ops import GROUP_LAYERS, T, cl, ncdhw, relerr
from test_gpu_precision import BAR, rms_rel

pytestmark = pytest.mark.gpu

_SKIPPED = []           # (test, budget) that met a device with no more CUs than the budget


@contextlib.contextmanager
def cu_budget(cus, what):
    """Plan for ``cus`` CUs inside the block; the device's count again after it, whatever happened."""
    from avid_hip import ops
    full = torch.cuda.get_device_properties(0).multi_processor_count
    if cus >= full:
        _SKIPPED.append((what, cus))
        pytest.skip(f"a budget of {cus} CUs is no reduction on a device of {full}")
    try:
        assert ops.set_cu_budget(cus) == cus
        yield
    finally:
        back = ops.set_cu_budget(0)
    assert back == full == ops.cu_budget()


def _out_shape(layer):
    cin, cout, k, stride, pad, (B, Ti, Hi, Wi) = R.LAYERS[layer]
    return (B, cout) + tuple((n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((Ti, Hi, Wi), pad, k, stride))


@functools.lru_cache(maxsize=None)
def _inputs(layer):
    """x, w (NCDHW) and the output gradient of a layer on the host: made once, never modified."""
    cin, cout, k, stride, pad, (B, Ti, Hi, Wi) = R.LAYERS[layer]
    x = T(detgen.det_normalish(f"budget:{layer}:x", (B, cin, Ti, Hi, Wi)))
    w = T(detgen.det_param(f"budget:{layer}:w.weight", (cout, cin) + k))
    gy = T(detgen.det_uniform(f"budget:{layer}:gy", _out_shape(layer)))
    return x, w, gy


@functools.lru_cache(maxsize=None)
def _reference(layer):
    """{"y" | "dx" | "dw": (float64 F.conv3d, float32 F.conv3d on the host)}: once per layer, shared by its budgets."""
    cin, cout, k, stride, pad, _ = R.LAYERS[layer]
    x, w, gy = _inputs(layer)
    out = []
    for dt in (torch.float64, torch.float32):
        xr, wr = x.to(dt, copy=True).requires_grad_(True), w.to(dt, copy=True).requires_grad_(True)
        yr = F.conv3d(xr, wr, stride=stride, padding=pad)
        (yr * gy.to(dt)).sum().backward()
        out.append((yr.detach(), xr.grad, wr.grad))
    return {q: (out[0][i], out[1][i]) for i, q in enumerate(("y", "dx", "dw"))}


def _run(layer, dev, bn_stats=False):
    """Forward + backward of a layer through ops.conv_cl under whatever budget is set: y, dx, dw (NCDHW views) [, partials]."""
    from avid_hip import ops
    cin, cout, k, stride, pad, _ = R.LAYERS[layer]
    x, w, gy = _inputs(layer)
    xd = cl(x).to(dev).requires_grad_(True)
    wd = ops.make_weight(cout, cin, *k)
    wd.copy_(w)
    wd = wd.to(dev).requires_grad_(True)
    out = ops.conv_cl(xd, wd, stride, pad, bn_stats=bn_stats)
    y, part = out if bn_stats else (out, None)
    y.backward(cl(gy).to(dev))
    torch.cuda.synchronize()
    res = {"y": ncdhw(y.detach()), "dx": ncdhw(xd.grad), "dw": wd.grad}
    if bn_stats:
        res["partials"] = part
    return res


@functools.lru_cache(maxsize=None)
def _full_run(layer, dev):
    """The layer at the device's full CU count (the budget tests call this BEFORE they set theirs) and the plans reported there."""
    from avid_hip import ops
    assert ops.cu_budget() == torch.cuda.get_device_properties(0).multi_processor_count
    return _run(layer, dev), R.names_now(layer)


def _check_partials(y_cl, part, cout):
    """test_conv_bn_partials' assertions on the partial rows: column totals == float64 column sums / sums of squares of y."""
    assert part.numel() > 0 and part.dim() == 3 and part.shape[1:] == (2, cout), tuple(part.shape)
    yd = y_cl.double().reshape(-1, cout)
    s, q = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
    e_s, e_q = relerr(s, yd.sum(0)), relerr(q, (yd * yd).sum(0))
    assert e_s < 1e-5 * max(1.0, float(yd.abs().sum(0).max() / (yd.sum(0).abs().max() + 1e-30))), e_s
    assert e_q < 1e-5, e_q
    return e_s, e_q


def _six_product(d, wgrad_name):
    """The outputs of a layer that six-product kernels compute (the kernels tests/test_gpu_precision.py
    lists): the implicit GEMM / tconv64_kernel on pre-split weights, wino2p_kernel, wgrad_tab_kernel / twgrad64_kernel."""
    return [q for q, on in (("y", d.split_fwd or d.wino_fwd == 2), ("dx", d.split_dgrad or d.wino_dgrad == 2),
                            ("dw", wgrad_name.startswith(("wgrad_tab_kernel", "twgrad64_kernel")))) if on]


def _bars(name, got, ref, six):
    """One `[budget]` line with every measured figure, then the bars: relerr for all, the rms bars for the outputs in ``six``."""
    rel = {q: relerr(got[q], ref[q][0]) for q in ("y", "dx", "dw") if q in got}
    rms = {q: (rms_rel(got[q], ref[q][0]), rms_rel(ref[q][1], ref[q][0])) for q in rel}
    print(f"\n[budget] {name}: " + ", ".join(
        f"{q} max {rel[q]:.2e} rms {rms[q][0]:.2e} (float32 conv3d {rms[q][1]:.2e}{'' if q in six else '; not six-product'})" for q in rel))
    for q, bar in (("y", 2e-5), ("dx", 2e-5), ("dw", 5e-5)):
        if q in rel:
            assert rel[q] < bar, (name, q, rel[q])
    for q in six:
        e_dev, e_f32 = rms[q]
        assert e_dev <= BAR, (name, q, e_dev)
        assert e_dev <= 3.0 * e_f32, (name, q, e_dev, e_f32)


@pytest.mark.parametrize("layer", [n for n in R.LAYERS if n not in R.CHAIN_LAYERS])
def test_full_budget_run_of_each_layer(layer, gpu_device, kernel_log):
    """The full-budget run the rows below are compared with, itself against float64 by the same bars."""
    from avid_hip import ops
    cin, cout, k, stride, pad, shp = R.LAYERS[layer]
    got, names = _full_run(layer, gpu_device)
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert names[:2] == tuple(R.FULL[layer]), names
    d = ops._desc_cached(shp, cin, cout, k, stride, pad, False)[0]
    six = _six_product(d, names[2])
    _bars(f"{layer}@full", got, _reference(layer), six)


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_rows_against_float64(row, gpu_device, kernel_log):
    from avid_hip import ops
    layer, budget = row[:2]
    cin, cout, k, stride, pad, shp = R.LAYERS[layer]
    ref = _reference(layer)
    full, full_names = _full_run(layer, gpu_device)
    fwd_classes = R.classes(layer, budget, 0, row[2])
    stats = bool(fwd_classes & R.STATS_CLASSES) or row[2].startswith("wino")
    with cu_budget(budget, R.row_id(row)):
        # the plan under the budget is the table's
        assert R.names_now(layer) == tuple(row[2:5])
        d, _, _, _, stats_rows = ops._desc_cached(shp, cin, cout, k, stride, pad, False)
        six = _six_product(d, row[4])
        with kernel_log() as log:
            got = _run(layer, gpu_device)
        again = _run(layer, gpu_device)
        with_stats = _run(layer, gpu_device, bn_stats=True) if stats else None
    # the launch log shows the families the plans name, and the reduce where a plan is K-split
    reduces = 0
    for name in row[2:5]:
        if name.startswith("wino_kernel<"):
            continue
        prefixes, reduce = R.family(name)
        for p in prefixes:
            assert log.launches(p) >= 1, (p, sorted(log.report))
        reduces += int(reduce)
    assert log.launches("splitk_reduce") >= reduces, (reduces, sorted(log.report))
    if row[2].startswith("wino_kernel<"):
        # (the plan names the family; which of its kernels a layer takes — wino_kernel, or wino2p_kernel from 1.5 rounds of
        #  64-tile units per planned CU — is avid_conv_uses_wino's answer under the budget)
        ran = {1: "wino_kernel", 2: "wino2p_kernel"}
        assert log.launches(ran[d.wino_fwd]) + (log.launches(ran[d.wino_dgrad]) if d.wino_dgrad != d.wino_fwd else 0) == 2, sorted(log.report)
        assert log.launches("wino_kernel") + log.launches("wino2_kernel") + log.launches("wino2p_kernel") == 2, sorted(log.report)
    else:
        assert log.launches("wino") == 0, sorted(log.report)
    _bars(R.row_id(row), got, ref, six)
    for q in ("y", "dx", "dw"):                                        # determinism
        assert torch.equal(got[q], again[q]), (R.row_id(row), q)
    # bit-identity to the full-budget run where both plans deal whole, unsplit tiles of the same kernel
    same = R.bit_identical_outputs(row, full_names)
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert same == R.bit_identical_outputs(row)
    for which, q in ((0, "y"), (1, "dx")):
        if which in same:
            assert torch.equal(got[q], full[q]), (R.row_id(row), q, float((got[q] - full[q]).abs().max()))
    if stats:
        assert torch.equal(with_stats["y"], got["y"])                # the statistics do not perturb the output
        if cout == 192:
            # three column blocks are 192 output channels, and avid_conv_fwd_stats_rows offers the epilogue only where Cout / 4
            # divides 256 (write_stats' lane map): by contract the layer answers 0 rows and conv_cl hands back an empty tensor —
            # write_stats' `slot % ntn` cannot meet ntn = 3.  Held to that answer, so that a change of the rule shows here.
            assert stats_rows == 0 and with_stats["partials"].numel() == 0
            return
        assert stats_rows > 0
        e_s, e_q = _check_partials(with_stats["y"].permute(0, 2, 3, 4, 1), with_stats["partials"], cout)
        print(f"[budget] {R.row_id(row)}: partial rows {tuple(with_stats['partials'].shape)}, column sums {e_s:.2e}, sums of squares {e_q:.2e}")


@pytest.mark.parametrize("row", R.CHAIN_ROWS, ids=R.row_id)
def test_bn_backward_partials_from_dgrad_under_budget(row, gpu_device, kernel_log):
    """test_bn_backward_partials_from_dgrad's chain (conv1 -> BN+ReLU -> conv2 [+ tap], the BatchNorm's backward sums out of
    conv2's input-gradient epilogue / K-split reduce) with conv2's input gradient on whole rounds + an unsplit tail, whole rounds
    + a K-split tail, and a weight-stationary tail: against the chain without the hand-over, 2e-5 of the gradient scale."""
    from avid_hip import ops
    layer, budget, dgrad = row
    cmid, cout, k, stride, pad, shape = R.LAYERS[layer]
    B, Ti, Hi, Wi = shape
    dev = gpu_device
    x = T(detgen.det_normalish(f"bnb:{shape}:x", (B, Ti, Hi, Wi, 64))).to(dev)
    w1 = ops.make_weight(cmid, 64, 1, 3, 3); w1.copy_(T(detgen.det_param(f"bnb:{cmid}:w1.weight", (cmid, 64, 1, 3, 3))))
    w2 = ops.make_weight(cout, cmid, *k); w2.copy_(T(detgen.det_param(f"bnb:{cout}:{k}:w2.weight", (cout, cmid) + k)))
    w1, w2 = w1.to(dev), w2.to(dev)
    gam = (T(detgen.det_uniform(f"bnb:{cmid}:g", (cmid,))) + 1.5).to(dev)
    bet = T(detgen.det_uniform(f"bnb:{cmid}:b", (cmid,))).to(dev)
    gy = T(detgen.det_uniform(f"bnb:{shape}:{cout}:gy", (B, Ti, Hi, Wi, cout))).to(dev)
    res, logs = {}, {}
    with cu_budget(budget, R.row_id(row)):
        assert R.names_now(layer)[1] == dgrad
        for fused in (False, True):
            for tap in (False, True):
                xx = x.clone().requires_grad_(True)
                g_, b_ = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
                rm, rv = torch.zeros(cmid, device=dev), torch.ones(cmid, device=dev)
                y1 = ops.conv_cl(xx, w1, (1, 1, 1), (0, 1, 1))
                src = ops.BnSource(None, None, True) if fused else None
                h = ops.batch_norm_cl(y1, g_, b_, rm, rv, True, relu=True, src=src)
                out = ops.conv_cl(h, w2, stride, pad, tap=tap, bn_src=src)
                y2, alias = (out[0], out[-1]) if tap else (out, None)
                loss = (y2 * gy).sum()
                if tap:
                    loss = loss + (alias * alias).sum() * 0.25
                with kernel_log() as log:
                    loss.backward()
                if fused:
                    assert src.partials is None                      # consumed by the BatchNorm's backward
                res[(fused, tap)] = (xx.grad.clone(), g_.grad.clone(), b_.grad.clone())
                logs[(fused, tap)] = log
    plan = R.parse(dgrad)
    for tap in (False, True):
        log = logs[(True, tap)]
        assert log.launches(dgrad.split(" ")[0]) >= 1, sorted(log.report)
        if plan["f"] > 1:        # the sums of the split rows come out of the reduce
            assert log.launches("splitk_reduce_bnb_kernel") >= 1, sorted(log.report)
        errs = [relerr(b, a) for a, b in zip(res[(False, tap)], res[(True, tap)])]
        print(f"\n[budget] {R.row_id(row)} tap={tap}: dx {errs[0]:.2e}, dgamma {errs[1]:.2e}, dbeta {errs[2]:.2e}")
        assert max(errs) < 2e-5, (R.row_id(row), tap, errs)


WINO_SHAPES = {64: (6, 8, 27, 29), 128: (5, 4, 45, 47)}


@functools.lru_cache(maxsize=None)
def _wino_case(ch):
    """Inputs and the float64 forward / backward of the ch -> ch (1,3,3) layer at WINO_SHAPES[ch], once for all its cases."""
    B, Ti, Hi, Wi = WINO_SHAPES[ch]
    x = T(detgen.det_normalish(f"budget:wino:{ch}:x", (B, Ti, Hi, Wi, ch)))
    w = T(detgen.det_param(f"budget:wino:{ch}:w.weight", (ch, ch, 1, 3, 3)))
    gy = T(detgen.det_uniform(f"budget:wino:{ch}:gy", (B, Ti, Hi, Wi, ch)))
    xr = x.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    wr = w.double().requires_grad_(True)
    yr = F.conv3d(xr, wr, padding=(0, 1, 1)).permute(0, 2, 3, 4, 1)
    (yr * gy.double()).sum().backward()
    return x, w, gy, yr.detach(), xr.grad.permute(0, 2, 3, 4, 1), wr.grad


@pytest.mark.parametrize("budget", [8, 24])
@pytest.mark.parametrize("kernel", ["wino_kernel", "wino2p_kernel"])
@pytest.mark.parametrize("ch", [64, 128])
def test_winograd_under_budget(ch, kernel, budget, gpu_device, kernel_log):
    """wino_kernel / wino2p_kernel, the input gradient through the same kernel and wino_wgrad_kernel with their grids cut to 8
    and 24 CUs: against float64 by test_winograd_random_shapes' bars, the BatchNorm partial rows by test_conv_bn_partials', and
    for wino2p_kernel bit-identical to the form that splits per use (test_wino2_presplit_is_bit_identical)."""
    from avid_hip import lib, ops
    x, w, gy, yr, dxr, dwr = _wino_case(ch)
    dev = gpu_device
    pre = lib.raw("avid_wino2_pre_configure")
    wino2 = kernel == "wino2p_kernel"
    res = {}
    ops.wino_configure(1, 1, 128)
    ops.wino2_configure(0 if wino2 else 100000)        # (by its own rule a small budget sends every layer to wino2p_kernel)
    try:
        with cu_budget(budget, f"wino:{ch}:{kernel}@{budget}"):
            for on in ((1, 0) if wino2 else (None,)):
                if on is not None:
                    pre(on)
                xd = x.to(dev).requires_grad_(True)
                wd = ops.make_weight(ch, ch, 1, 3, 3)
                wd.copy_(w)
                wd = wd.to(dev).requires_grad_(True)
                with kernel_log() as log:
                    y, part = ops.conv_cl(xd, wd, (1, 1, 1), (0, 1, 1), bn_stats=True)
                    y.backward(gy.to(dev))
                ran = kernel if on != 0 else "wino2_kernel"
                others = {"wino_kernel", "wino2_kernel", "wino2p_kernel"} - {ran}
                assert log.launches(ran) == 2 and log.launches("wino_wgrad_kernel") == 1, sorted(log.report)
                assert all(log.launches(o) == 0 for o in others), sorted(log.report)
                res[on] = (y.detach(), part.clone(), xd.grad, wd.grad)
    finally:
        pre(-1)
        ops.wino_configure(-1, -1, -1)
        ops.wino2_configure(-1)
    y, part, dx, dw = res[1 if wino2 else None]
    errs = (relerr(y, yr), relerr(dx, dxr), relerr(dw, dwr))
    print(f"\n[budget] wino {ch} ch {kernel}@{budget}: y max {errs[0]:.2e}, dx max {errs[1]:.2e}, dw max {errs[2]:.2e}")
    assert errs[0] < 2e-5 and errs[1] < 2e-5 and errs[2] < 5e-5, errs
    _check_partials(y, part, ch)
    if wino2:
        for a, b in zip(res[1], res[0]):
            assert torch.equal(a, b)


# which -> (Cin, k, stride, pad, shape, forward kernel, weight-gradient kernel).  The LDS-patch stem kernels want an input width
# that is a multiple of 4 (stem_fwd_supported): the 65-wide spectrogram goes to igemm_gather_kernel / wgrad_gather_kernel, which
# write no BatchNorm partial rows (conv_cl hands back an empty tensor, its documented answer); its 64-wide twin runs
# stem_fwd_kernel<1,1> / stem_wgrad_kernel<1,1>, whose grid and group count are the budget's
STEMS = {"video": (3, (3, 7, 7), (1, 2, 2), (1, 3, 3), (2, 3, 8, 56, 56), "stem_fwd3", "stem_wgrad"),
         "audio": (1, (1, 7, 7), (1, 2, 2), (0, 3, 3), (4, 1, 1, 50, 65), "igemm_gather_kernel", "wgrad_gather_kernel"),
         "audio_w64": (1, (1, 7, 7), (1, 2, 2), (0, 3, 3), (4, 1, 1, 50, 64), "stem_fwd_kernel<1,1>", "stem_wgrad_kernel<1,1>")}


@functools.lru_cache(maxsize=None)
def _stem_case(which):
    cin, k, stride, pad, shp = STEMS[which][:5]
    x = T(detgen.det_normalish(f"budget:stem:{which}:x", shp))
    w = T(detgen.det_param(f"budget:stem:{which}:w.weight", (64, cin) + k))
    wr = w.double().requires_grad_(True)
    yr = F.conv3d(x.double(), wr, stride=stride, padding=pad)
    gy = T(detgen.det_uniform(f"budget:stem:{which}:gy", tuple(yr.shape)))
    (yr * gy.double()).sum().backward()
    return x, w, gy, yr.detach(), wr.grad


def _stem_run(which, dev):
    from avid_hip import ops
    cin, k, stride, pad = STEMS[which][:4]
    x, w, gy = _stem_case(which)[:3]
    wd = ops.make_weight(64, cin, *k)
    wd.copy_(w)
    wd = wd.to(dev).requires_grad_(True)
    y, part = ops.conv_cl(x.to(dev), wd, stride, pad, channel_first=True, bn_stats=True)
    y.backward(cl(gy).to(dev))
    torch.cuda.synchronize()
    return y.detach(), part, wd.grad


@functools.lru_cache(maxsize=None)
def _stem_full(which, dev):
    return _stem_run(which, dev)


@pytest.mark.parametrize("budget", [8, 24])
@pytest.mark.parametrize("which", list(STEMS))
def test_stem_under_budget(which, budget, gpu_device, kernel_log):
    """The stems' grids and the weight gradient's groups follow the budget: forward and weight gradient against float64 by
    test_stem_conv's bars, the partial rows by test_stem_bn_partials' assertion — and the forward output is the full-budget
    run's bits (the stem's outputs do not depend on the grid, only the order of its partial sums does)."""
    x, w, gy, yr, dwr = _stem_case(which)
    fwd_kernel, wgrad_kernel = STEMS[which][5:]
    y_full = _stem_full(which, gpu_device)[0]
    with cu_budget(budget, f"stem:{which}@{budget}"):
        with kernel_log() as log:
            y, part, dw = _stem_run(which, gpu_device)
        y_again, part_again, dw_again = _stem_run(which, gpu_device)
    assert log.launches(fwd_kernel) == 1 and log.launches(wgrad_kernel) == 1, sorted(log.report)
    e_y, e_dw = relerr(ncdhw(y), yr), relerr(dw, dwr)
    print(f"\n[budget] stem {which}@{budget}: y max {e_y:.2e}, dw max {e_dw:.2e}, partial rows {tuple(part.shape)}")
    assert e_y < 2e-5 and e_dw < 5e-5, (e_y, e_dw)
    assert torch.equal(y, y_full)
    assert torch.equal(y, y_again) and torch.equal(part, part_again) and torch.equal(dw, dw_again)
    if fwd_kernel == "igemm_gather_kernel":         # no LDS-patch stem kernel, no conv-side partial rows: see STEMS
        assert part.numel() == 0
        return
    assert part.shape[0] >= 1
    _check_partials(y, part, 64)


@functools.lru_cache(maxsize=None)
def _group_case():
    """GROUP_LAYERS[:12]: inputs and float64 weight gradients, once for both budgets."""
    out = []
    for i, (cin, cout, k, stride, pad, (B, Ti, Hi, Wi)) in enumerate(GROUP_LAYERS[:12]):
        x = T(detgen.det_normalish(f"grp:{i}:x", (B, cin, Ti, Hi, Wi)))
        w = T(detgen.det_param(f"grp:{i}:w.weight", (cout, cin) + k))
        wr = w.double().requires_grad_(True)
        yr = F.conv3d(x.double(), wr, stride=stride, padding=pad)
        gy = T(detgen.det_uniform(f"grp:{i}:gy", tuple(yr.shape)))
        (yr * gy.double()).sum().backward()
        out.append((cl(x), cl(gy), wr.grad))
    return out


@pytest.mark.parametrize("budget", [8, 24])
def test_grouped_weight_gradients_under_budget(budget, gpu_device, kernel_log):
    """avid_conv_wgrad_group with plan_group's workgroup slots cut to 16 and 48 (two per CU): every layer against float64 by
    test_grouped_weight_gradients' bar (5e-5 of each gradient's scale), a second launch bit-identical, and the form that
    splits its fragments once at the LDS write bit-identical to the one that splits per use."""
    import ctypes as C
    from avid_hip import lib, ops
    dev = gpu_device
    layers = GROUP_LAYERS[:12]
    count = len(layers)
    pre = lib.raw("avid_wgrad_pre_configure")
    res = {}
    try:
        with cu_budget(budget, f"wgrad_group@{budget}"):
            items = (lib.WgradItem * count)()
            keep, outs = [], []
            for i, ((cin, cout, k, stride, pad, shp), (x, gy, _)) in enumerate(zip(layers, _group_case())):
                xd, gyd = x.to(dev), gy.to(dev)
                d = ops._desc_cached(shp, cin, cout, k, stride, pad, False)[0]
                assert d.groupable
                dw = ops.make_weight(cout, cin, *k).to(dev)
                items[i].d = d
                items[i].x, items[i].dy, items[i].dw = xd.data_ptr(), gyd.data_ptr(), dw.data_ptr()
                keep += [xd, gyd]
                outs.append(dw)
            nb = lib.raw("avid_conv_wgrad_group_workspace_bytes")(count, items)
            ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)
            for on in (1, 0, 1):
                pre(on)
                for o in outs:
                    o.fill_(float("nan"))                              # every element must be written
                with kernel_log() as log:
                    lib.call("avid_conv_wgrad_group", count, items, ops._p(ws), ws.numel(), ops._stream())
                assert log.launches("wgrad_group_kernel") == 1, sorted(log.report)
                res.setdefault(on, []).append([o.clone() for o in outs])
    finally:
        pre(-1)
    worst = 0.0
    for i, (_, _, ref) in enumerate(_group_case()):
        first, second = res[1][0][i], res[1][1][i]
        e = relerr(first, ref)
        worst = max(worst, e)
        assert e < 5e-5, (i, e)
        assert torch.equal(first, second), i
        assert torch.equal(first, res[0][0][i]), (i, float((first - res[0][0][i]).abs().max()))
    print(f"\n[budget] wgrad_group@{budget}: worst dw max {worst:.2e} over {count} layers")


def test_zz_no_budget_was_skipped_on_a_full_chip(gpu_device):
    """Last in the module: on a 256-CU MI355X every budget above is a reduction, so none of the cases may have skipped."""
    if torch.cuda.get_device_properties(0).multi_processor_count >= 256:
        assert _SKIPPED == []
