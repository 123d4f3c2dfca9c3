"""The kernel that runs is the kernel named: for one smallest layer per kernel family, forward, input gradient and weight
gradient run through ``ops`` with the planned workspace, and the launch log (the library's HIP-event timers) holds exactly the
kernels ``avid_conv_kernel_name`` names — family and template arguments, and the reduce / scatter kernels behind them — and no
other convolution kernel.  Outputs against float64 ``F.conv3d`` with the bars of tests/test_gpu_ops.py (2e-5 / 2e-5 / 5e-5 of the
largest reference magnitude for y / dx / dw).

Queries and launches read one decision (csrc/conv.hip conv_route); tests/test_conv_routes_host.py pins the queries'
answers on the host, this test that the launches follow them."""
import ctypes as C
import functools
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import detgen
from test_gpu_ops import T, cl, ncdhw, relerr

pytestmark = pytest.mark.gpu

S1 = (1, 1, 1)
# name -> (Cin, Cout, k, stride, pad, (B, T, H, W), channel_first, switches)
CASES = {
    # (the persistent kernel's 128 x 128 tile: at 256 CUs the planner gives the first shape the 128 x 64 tile — 156 units against
    #  78 on 512 slots; the smallest layer of the benchmark's list that gets the wide tile stands for it)
    "pk_dense": (64, 128, (1, 3, 3), S1, (0, 1, 1), (2, 4, 14, 14), False, {"wino": 0}),
    "pk_128x128": (128, 128, (1, 3, 3), S1, (0, 1, 1), (1, 8, 28, 28), False, {"wino": 0}),
    "pk_128x64": (128, 64, (3, 1, 1), S1, (1, 0, 0), (1, 4, 7, 7), False, {}),
    "wino": (64, 128, (1, 3, 3), S1, (0, 1, 1), (2, 4, 14, 14), False, {"wino": 1}),
    "tconv": (64, 64, (3, 1, 1), S1, (1, 0, 0), (1, 8, 13, 15), False, {"tconv": 2}),
    "strided": (64, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 7, 13, 15), False, {}),    # odd extents: every parity class uneven
    "compact": (64, 128, (1, 1, 1), (1, 2, 2), (0, 0, 0), (1, 7, 13, 15), False, {}),
    "video_stem": (3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3), (1, 8, 32, 32), True, {}),
    "audio_stem": (1, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), (1, 1, 40, 100), True, {}),
    "gather": (16, 64, (1, 3, 3), S1, (0, 1, 1), (1, 4, 14, 14), True, {}),
}
# the family each case is there for: a prefix of the forward / input gradient / weight gradient name (None: no such gradient)
WANT = {
    "pk_dense": ("igemm_pk_kernel<", "igemm_pk_kernel<", "wgrad_tab_kernel<2,2>"),
    "pk_128x128": ("igemm_pk_kernel<4,1,1,4,0>", "igemm_pk_kernel<4,1,1,4,1>", "wgrad_tab_kernel<2,2>"),
    "pk_128x64": ("igemm_pk_kernel<4,1,1,2,0>", "igemm_pk_kernel<4,1,1,2,1>", "wgrad_tab_kernel<1,3>"),
    "wino": ("wino_kernel<0>", "wino_kernel<1>", "wino_wgrad_kernel"),
    "tconv": ("tconv64_kernel<0>", "tconv64_kernel<1>", "twgrad64_kernel"),
    "strided": ("igemm_pk_kernel<4,1,1,2,0>", "igemm_pk_kernel<4,1,1,2,1>s2", "wgrad_tab_kernel<2,2>"),
    "compact": ("igemm_pk_kernel<4,1,1,2,0>", "igemm_pk_kernel over the sub-sampled grid + dx_scatter_strided_kernel", "wgrad_tab_kernel<2,2>"),
    "video_stem": ("stem_fwd3p_kernel<3,3>", "stem_dgrad_kernel<3,3>", "stem_wgrad_kernel"),
    "audio_stem": ("stem_fwd", "stem_dgrad_kernel<1,1>", "stem_wgrad_kernel"),
    "gather": ("igemm_gather_kernel<2,2,1,1>", None, "wgrad_gather_kernel"),
}
# every convolution kernel's timer name starts with one of these (weight preparation — transposes, transforms — does not)
CONV_KERNELS = ("igemm_", "tconv64", "twgrad64", "wino_kernel", "wino2", "wino_wgrad", "stem_", "wgrad_tab", "wgrad_gather",
                "wgrad_group", "wgrad_reduce", "splitk_reduce", "dx_scatter")
PK = re.compile(r"(igemm_pk_kernel<[\d,]+>) full=\d+ tail_units=\d+ f=(\d+)")


def expected_launches(name, which, d):
    """The launch log a reported name stands for: {timer name, or prefix*suffix: (fewest, most) launches}.  Where the name does
    not say whether a reduce follows (a strided plan splits K per class, a Winograd weight gradient may split the pixels) both
    are allowed."""
    m = PK.match(name)
    if m:
        return {m.group(1): (1, 1), "splitk_reduce*": (1, 1) if int(m.group(2)) > 1 else (0, 0)}
    if name.startswith("igemm_pk_kernel over the sub-sampled grid"):      # the compact descriptor's input gradient + the scatter
        return {"igemm_pk_kernel<*,1>": (1, 1), "dx_scatter_strided_kernel": (1, 1), "splitk_reduce*": (0, 1)}
    if "s2 (stride-parity classes)" in name:
        return {name.split(" ")[0]: (1, 1), "splitk_reduce*": (0, 1)}
    if name.startswith("wino_kernel<"):        # the family; which of its kernels: avid_conv_uses_wino
        return {{1: "wino_kernel<*", 2: "wino2*"}[d.wino_fwd if which == 0 else d.wino_dgrad]: (1, 1)}
    if name.startswith("tconv64_kernel<"):
        return {name.split(" ")[0]: (1, 1)}
    if name.startswith("twgrad64_kernel"):
        return {"twgrad64_kernel": (1, 1), "wgrad_reduce*": (1, 1)}
    if name == "wino_wgrad_kernel":
        return {"wino_wgrad_kernel": (1, 1), "wgrad_reduce*": (0, 1)}
    m = re.match(r"(wgrad_tab_kernel<\d,\d>|wgrad_gather_kernel) splits=(\d+)$", name)
    if m:
        return {m.group(1): (1, 1), "wgrad_reduce*": (1, 1) if int(m.group(2)) > 1 else (0, 0)}
    if name.startswith("stem_wgrad_kernel"):
        return {"stem_wgrad*": (1, 1)}
    return {name: (1, 1)}                      # stems, gather: the name is the timer's


def launches(log, pattern):
    """Launches under an exact timer name, a prefix ("...*") or a prefix and suffix ("...*...")."""
    if "*" not in pattern:
        return log.report.get(pattern, {"launches": 0})["launches"]
    pre, suf = pattern.split("*")
    return sum(v["launches"] for n, v in log.report.items() if n.startswith(pre) and n.endswith(suf))


@functools.lru_cache(maxsize=None)
def _data(case):
    """x, w (NCDHW), the output gradient and the float64 y / dx / dw of a case, on the host: made once, never modified."""
    cin, cout, k, stride, pad, (B, Ti, Hi, Wi), cf, _ = CASES[case]
    x = T(detgen.det_normalish(f"routes:{case}:x", (B, cin, Ti, Hi, Wi)))
    w = T(detgen.det_param(f"routes:{case}:w.weight", (cout, cin) + k))
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv3d(xr, wr, stride=stride, padding=pad)
    gy = T(detgen.det_uniform(f"routes:{case}:gy", tuple(yr.shape)))
    (yr * gy.double()).sum().backward()
    return x, w, gy, yr.detach(), xr.grad, wr.grad


@pytest.fixture
def switches():
    """Sets a case's dispatch switches; the defaults again afterwards, whatever happened."""
    from avid_hip import ops

    def set_(sw):
        if "wino" in sw:
            ops.wino_configure(sw["wino"], 1 if sw["wino"] else -1, -1)
        if "tconv" in sw:
            ops.tconv_configure(sw["tconv"])
    yield set_
    ops.wino_configure(-1, -1, -1)
    ops.tconv_configure(-1)


def _names(d):
    from avid_hip import lib
    buf = C.create_string_buffer(256)
    out = []
    for which in (0, 1, 2):
        rc = lib.raw("avid_conv_kernel_name")(C.byref(d), which, buf, 256)
        out.append(buf.value.decode() if rc == 0 else None)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_the_launch_log_is_what_the_name_query_names(case, gpu_device, kernel_log, switches):
    from avid_hip import ops
    cin, cout, k, stride, pad, shp, cf, sw = CASES[case]
    x, w, gy, y64, dx64, dw64 = _data(case)
    switches(sw)
    d = ops._desc_cached(shp, cin, cout, k, stride, pad, cf)[0]
    names = _names(d)
    for got, want in zip(names, WANT[case]):          # the case reaches the family it is there for
        assert (got is None) == (want is None) and (got is None or got.startswith(want)), (case, names)
    has_dx = names[1] is not None
    xd = (x if cf else cl(x)).to(gpu_device).requires_grad_(has_dx)
    wd = ops.make_weight(cout, cin, *k)
    wd.copy_(w)
    wd = wd.to(gpu_device).requires_grad_(True)
    ops.conv_cl(xd, wd, stride, pad, channel_first=cf).backward(cl(gy).to(gpu_device))     # (weight tables made, workspaces grown)
    xd.grad = wd.grad = None
    with kernel_log() as log:
        y = ops.conv_cl(xd, wd, stride, pad, channel_first=cf)
        y.backward(cl(gy).to(gpu_device))
    want = {}                                  # the three directions' launches, pooled by timer (two may share one)
    for which, name in enumerate(names):
        for t, (lo, hi) in (expected_launches(name, which, d) if name else {}).items():
            want[t] = (want.get(t, (0, 0))[0] + lo, want.get(t, (0, 0))[1] + hi)
    for t, (lo, hi) in want.items():
        assert lo <= launches(log, t) <= hi, (case, t, (lo, hi), names, sorted(log.report))
    kernels = sum(launches(log, t) for t in want)
    # ... and nothing else: every convolution kernel in the log is accounted for
    seen = sum(v["launches"] for n, v in log.report.items() if n.startswith(CONV_KERNELS))
    assert seen == kernels, (case, names, {n: v["launches"] for n, v in log.report.items()})
    errs = {"y": relerr(ncdhw(y.detach()), y64), "dw": relerr(wd.grad, dw64)}
    if has_dx:
        errs["dx"] = relerr(xd.grad if cf else ncdhw(xd.grad), dx64)
    print(f"\n[routes] {case}: {names} " + ", ".join(f"{q} {e:.2e}" for q, e in errs.items()))
    for q, bar in (("y", 2e-5), ("dx", 2e-5), ("dw", 5e-5)):
        if q in errs:
            assert errs[q] < bar, (case, q, errs[q])


def test_tconv_with_the_batchnorm_in_front_of_it(gpu_device, kernel_log, switches):
    """The in-affine form of the tconv64 / twgrad64 case: avid_conv_takes_in_affine says 1, the fused kernels run (and only
    they), y and dw against float64 of conv(ReLU(x * scale + shift))."""
    from avid_hip import ops
    cin, cout, k, stride, pad, shp, cf, sw = CASES["tconv"]
    x, w, gy, *_ = _data("tconv")
    switches(sw)
    d = ops._desc_cached(shp, cin, cout, k, stride, pad, cf)[0]
    names = _names(d)
    assert d.in_affine and names[0].startswith("tconv64_kernel<0>") and names[2].startswith("twgrad64_kernel"), names
    scale = T(detgen.det_uniform("routes:aff:scale", (64,)) * 3.0 - 1.0)
    shift = T(detgen.det_uniform("routes:aff:shift", (64,)) - 0.5)
    zr = torch.relu(x.double() * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1))
    wr = w.double().requires_grad_(True)
    yr = F.conv3d(zr, wr, stride=stride, padding=pad)
    (yr * gy.double()).sum().backward()
    xd, dy = cl(x).to(gpu_device), cl(gy).to(gpu_device)
    wd = ops.make_weight(cout, cin, *k)
    wd.copy_(w)
    wd = wd.to(gpu_device)
    sc, sh = scale.to(gpu_device), shift.to(gpu_device)
    ops.conv_fwd_in(xd, wd, stride, pad, sc, sh)                    # (weight table made)
    with kernel_log() as log:
        y = ops.conv_fwd_in(xd, wd, stride, pad, sc, sh)
        dw = ops.conv_wgrad_in(xd, dy, wd, stride, pad, sc, sh)
    assert log.launches("tconv64_kernel<0>") == 1 and log.launches("twgrad64_kernel") == 1 and log.launches("wgrad_reduce") == 1
    assert sum(v["launches"] for n, v in log.report.items() if n.startswith(CONV_KERNELS)) == 3, sorted(log.report)
    e_y, e_dw = relerr(ncdhw(y), yr.detach()), relerr(dw, wr.grad)
    print(f"\n[routes] tconv in-affine: y {e_y:.2e}, dw {e_dw:.2e}")
    assert e_y < 2e-5 and e_dw < 5e-5
