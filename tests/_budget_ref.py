"""(layer, CU budget) -> the plans ``avid_conv_kernel_name`` reports, shared by tests/test_cu_budget_host.py (pins the table
on the host) and tests/test_gpu_cu_budget.py (runs every row against float64).

A plan for a budget below the device's CU count does not depend on the device (csrc/common.hip device_cus), and without a
GPU the library plans for 256 physical CUs: the table is the same on the host and on a 256-CU MI355X.  Run as a script
(``python tests/_budget_ref.py``) this module prints the table as the library reports it, one JSON line per row: that is
how the host test reads it in a process of its own (the budget is process-global), and how the table is re-enumerated.

The classes (plan_pk_tile, csrc/conv.hip) are told from the reported plan, the budget and the layer's column count:
 (a) whole rounds only, `full` no multiple of the grid       (f) the 4,1,1,4 tile with whole rounds
 (b) whole rounds + an unsplit tail                          (g) three column blocks
 (c) whole rounds + a K-split tail (reduce)                  (h) a compact grid: full + tail_units <= C / 2
 (d) no whole round, K-split, weight-stationary order        (i) a single tail unit
 (e) no whole round, K-split, tile-major order
"""
import re

S1 = (1, 1, 1)
# name -> (Cin, Cout, k, stride, pad, (B, T, H, W)), channels-last
LAYERS = {
    "s64": (64, 64, (1, 3, 3), S1, (0, 1, 1), (3, 4, 20, 21)),
    "t128": (128, 128, (3, 1, 1), S1, (1, 0, 0), (3, 4, 14, 13)),
    "t256": (256, 256, (3, 1, 1), S1, (1, 0, 0), (6, 2, 7, 9)),
    "s128": (128, 128, (1, 3, 3), S1, (0, 1, 1), (9, 4, 14, 13)),
    "s64_192": (64, 192, (1, 3, 3), S1, (0, 1, 1), (2, 2, 15, 17)),
    "s192_64": (192, 64, (1, 3, 3), S1, (0, 1, 1), (2, 2, 15, 17)),
    "s64_small": (64, 64, (1, 3, 3), S1, (0, 1, 1), (2, 3, 9, 11)),
    "s64_333": (64, 64, (3, 3, 3), S1, (1, 1, 1), (2, 3, 11, 13)),
    "s256": (256, 256, (1, 3, 3), S1, (0, 1, 1), (4, 2, 7, 7)),
    "s512": (512, 512, (1, 3, 3), S1, (0, 1, 1), (8, 1, 4, 4)),
    "t64": (64, 64, (3, 1, 1), S1, (1, 0, 0), (1, 8, 27, 29)),
    "t64_tiny": (64, 64, (3, 1, 1), S1, (1, 0, 0), (1, 2, 9, 11)),
    "s2_spatial": (64, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 4, 18, 20)),
    "s2_temporal": (128, 128, (3, 1, 1), (2, 1, 1), (1, 0, 0), (2, 4, 9, 10)),
    "s2_res": (64, 128, (1, 1, 1), (2, 2, 2), (0, 0, 0), (2, 4, 10, 12)),
    "wino256": (256, 256, (1, 3, 3), S1, (0, 1, 1), (8, 2, 21, 19)),
}

PK = "igemm_pk_kernel<4,1,1,2,%d> "
PKW = "igemm_pk_kernel<4,1,1,4,%d> "
S2 = "igemm_pk_kernel<4,1,1,2,1>s2 (stride-parity classes)"
WS = " weight-stationary"


def _both(fmt, plan):
    return fmt % 0 + plan, fmt % 1 + plan


# (layer, budget, forward, input gradient, weight gradient)
ROWS = [
    ("s64", 8) + _both(PK, "full=40 tail_units=0 f=1") + ("wgrad_tab_kernel<1,3> splits=32",),          # ragged whole rounds, G = 16
    ("s64", 24) + _both(PK, "full=24 tail_units=16 f=1") + ("wgrad_tab_kernel<1,3> splits=32",),        # rounds + unsplit tail
    ("s64", 16) + _both(PK, "full=32 tail_units=16 f=2") + ("wgrad_tab_kernel<1,3> splits=32",),        # rounds + K-split tail + reduce
    ("t128", 16) + _both(PK, "full=32 tail_units=16 f=4") + ("wgrad_tab_kernel<2,2> splits=14",),       # the same, three taps
    ("t128", 8) + _both(PK, "full=32 tail_units=4 f=1") + ("wgrad_tab_kernel<2,2> splits=14",),
    ("t256", 16) + _both(PK, "full=16 tail_units=16 f=2") + ("wgrad_tab_kernel<2,2> splits=6",),        # four column blocks
    ("s128", 24) + _both(PKW, "full=48 tail_units=24 f=6") + ("wgrad_tab_kernel<2,2> splits=41",),      # 128 x 128 tile, rounds + split tail
    # three column blocks, G = 30: the unpaired xcd_remap with G % 8 != 0 — forward of 64 -> 192, input gradient of 192 -> 64;
    # the other direction of each is a weight-stationary tail
    ("s64_192", 16, PK % 0 + "full=15 tail_units=9 f=1", PK % 1 + "full=0 tail_units=16 f=2" + WS, "wgrad_tab_kernel<1,3> splits=8"),
    ("s192_64", 16, PK % 0 + "full=0 tail_units=16 f=2" + WS, PK % 1 + "full=15 tail_units=9 f=1", "wgrad_tab_kernel<1,3> splits=8"),
    ("s64_small", 16) + _both(PK, "full=0 tail_units=15 f=3" + WS) + ("wgrad_tab_kernel<1,3> splits=4",),     # stationary, small grid
    ("s64_333", 24) + _both(PK, "full=0 tail_units=21 f=3" + WS) + ("wgrad_tab_kernel<1,3> splits=6",),       # 27 taps
    ("s256", 40) + _both(PKW, "full=0 tail_units=40 f=5" + WS) + ("wgrad_tab_kernel<2,2> splits=3",),         # 128 x 128 tile, stationary
    ("s512", 16) + _both(PKW, "full=0 tail_units=16 f=4") + ("wgrad_tab_kernel<2,2> splits=1",),              # K = 4608, tile-major
    ("t64", 24) + _both(PK, "full=48 tail_units=1 f=1") + ("wgrad_tab_kernel<1,3> splits=49",),               # a single tail unit
    # tconv64_kernel / twgrad64_kernel by the default rule (three rounds of tiles at 8 CUs), nothing forced
    ("t64", 8, "tconv64_kernel<0> grid=7", PK % 1 + "full=48 tail_units=1 f=1", "twgrad64_kernel grid=7"),
    ("t64_tiny", 8) + _both(PK, "full=0 tail_units=2 f=1") + ("wgrad_tab_kernel<1,3> splits=1",),             # compact grid, both directions
    # plan_strided under a budget
    ("s2_spatial", 8, PKW % 0 + "full=0 tail_units=6 f=1", S2, "wgrad_tab_kernel<2,2> splits=5"),
    ("s2_spatial", 16, PK % 0 + "full=0 tail_units=12 f=1", S2, "wgrad_tab_kernel<2,2> splits=5"),
    ("s2_temporal", 8, PK % 0 + "full=0 tail_units=6 f=1", S2, "wgrad_tab_kernel<2,2> splits=3"),
    ("s2_res", 8, PK % 0 + "full=0 tail_units=2 f=1", "igemm_pk_kernel over the sub-sampled grid + dx_scatter_strided_kernel",
     "wgrad_tab_kernel<2,2> splits=1"),                                                                       # compact grid
    # the Winograd grid follows the budget
    ("wino256", 8, "wino_kernel<0> grid=8", "wino_kernel<1> grid=8", "wino_wgrad_kernel"),
    ("wino256", 24, "wino_kernel<0> grid=24", "wino_kernel<1> grid=24", "wino_wgrad_kernel"),
]

# the same layers at every CU of a 256-CU device (what the library plans without a GPU too): forward, input gradient
FULL = {
    "s64": _both(PK, "full=0 tail_units=240 f=6"),
    "t128": _both(PK, "full=0 tail_units=144 f=4"),
    "t256": _both(PK, "full=0 tail_units=192 f=8" + WS),
    "s128": _both(PK, "full=0 tail_units=208 f=2"),
    "s64_192": (PK % 0 + "full=0 tail_units=144 f=6" + WS, PK % 1 + "full=0 tail_units=144 f=18"),
    "s192_64": (PK % 0 + "full=0 tail_units=144 f=18", PK % 1 + "full=0 tail_units=144 f=6" + WS),
    "s64_small": _both(PK, "full=0 tail_units=30 f=6"),
    "s64_333": _both(PK, "full=0 tail_units=126 f=18" + WS),
    "s256": _both(PK, "full=0 tail_units=240 f=15" + WS),
    "s512": _both(PK, "full=0 tail_units=232 f=29"),
    "t64": _both(PK, "full=0 tail_units=49 f=1"),
    "t64_tiny": _both(PK, "full=0 tail_units=2 f=1"),
    "s2_spatial": (PK % 0 + "full=0 tail_units=72 f=6" + WS, S2),
    "s2_temporal": (PK % 0 + "full=0 tail_units=24 f=4", S2),
    "s2_res": (PK % 0 + "full=0 tail_units=2 f=1", "igemm_pk_kernel over the sub-sampled grid + dx_scatter_strided_kernel"),
    "wino256": ("wino_kernel<0> grid=220", "wino_kernel<1> grid=220"),
}

# conv -> BN+ReLU -> conv (test_bn_backward_partials_from_dgrad's 64- and 128-channel stride-1 shapes): the input-gradient plan of
# the second convolution, which also makes the BatchNorm's backward sums — classes (c), (d) and (b), (c)
CHAIN_LAYERS = {
    "chain64": (64, 64, (1, 3, 3), S1, (0, 1, 1), (2, 4, 12, 12)),
    "chain128": (128, 128, (1, 3, 3), S1, (0, 1, 1), (4, 3, 17, 19)),
}
LAYERS.update(CHAIN_LAYERS)
CHAIN_ROWS = [
    ("chain64", 8, PK % 1 + "full=8 tail_units=6 f=6"),
    ("chain64", 24, PK % 1 + "full=0 tail_units=18 f=2" + WS),
    ("chain128", 8, PKW % 1 + "full=24 tail_units=7 f=1"),
    ("chain128", 24, PKW % 1 + "full=24 tail_units=21 f=3"),
]
# classes whose forward rows also run with the BatchNorm-statistics epilogue (write_stats' owner column block, pk_rot, pk_ws)
STATS_CLASSES = set("abcdgi")


def row_id(row):
    return f"{row[0]}@{row[1]}"


def bit_identical_outputs(row, full_names=None):
    """Which of (0: y, 1: dx) must be the full-budget run's bits: both plans unsplit (f = 1) on the same kernel template, and the
    row neither a tconv64 nor a Winograd one — a whole tile has the same contraction order wherever it is dealt.
    ``full_names``: the plans reported at the device's full count (default: the 256-CU plans of FULL)."""
    if any(n.startswith(("tconv64", "twgrad64", "wino")) for n in row[2:5]):
        return set()
    out = set()
    for which in (0, 1):
        a, b = parse(row[2 + which]), parse((full_names or FULL[row[0]])[which])
        if a and b and a["f"] == 1 and b["f"] == 1 and a["tile"] == b["tile"]:
            out.add(which)
    return out


def parse(name):
    """An igemm_pk_kernel plan string -> dict(tile, mode, full, tail, f, ws), or None for another family."""
    m = re.match(r"igemm_pk_kernel<(\d,\d,\d,\d),(\d)> full=(\d+) tail_units=(\d+) f=(\d+)( weight-stationary)?$", name)
    if not m:
        return None
    return {"tile": m.group(1), "mode": int(m.group(2)), "full": int(m.group(3)), "tail": int(m.group(4)), "f": int(m.group(5)),
            "ws": bool(m.group(6))}


def classes(layer, budget, which, name):
    """The classes (a)-(i) of the module docstring a reported plan belongs to (empty for the other kernel families)."""
    p = parse(name)
    if p is None:
        return set()
    cin, cout = LAYERS[layer][:2]
    cd = cout if which == 0 else cin
    ntn = cd // (64 if p["tile"] == "4,1,1,2" else 128)
    c = budget // ntn * ntn or ntn                   # plan_pk_tile's C; the grid is 2 C workgroups unless compact
    full, tail, f = p["full"], p["tail"], p["f"]
    out = set()
    if full > 0 and tail == 0 and full % (2 * c):
        out.add("a")
    if full > 0 and tail > 0 and f == 1:
        out.add("b")
    if full > 0 and f > 1:
        out.add("c")
    if full == 0 and f > 1:
        out.add("d" if p["ws"] else "e")
    if p["tile"] == "4,1,1,4" and full > 0:
        out.add("f")
    if ntn == 3:
        out.add("g")
    if full + tail <= c // 2:
        out.add("h")
    if tail == 1:
        out.add("i")
    return out


def family(name):
    """The launch-log prefixes (tests/conftest.py kernel_log) a reported plan must show, and whether a K-split reduce follows."""
    if name.startswith("igemm_pk_kernel over the sub-sampled grid"):
        return ["igemm_pk_kernel", "dx_scatter_strided_kernel"], False
    p = parse(name)
    return [name.split(" ")[0]], bool(p and p["f"] > 1)


def names_now(layer):
    """(forward, input gradient, weight gradient) of a layer as the library reports them under the budget set in THIS process."""
    import ctypes as C
    from avid_hip import lib, ops
    cin, cout, k, stride, pad, shp = LAYERS[layer]
    d = ops._desc(shp, cin, cout, k, stride, pad, False)
    buf = C.create_string_buffer(256)
    names = []
    for which in (0, 1, 2):
        assert lib.raw("avid_conv_kernel_name")(C.byref(d), which, buf, 256) == 0
        names.append(buf.value.decode())
    return tuple(names)


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avid-cma_amd"))
    from avid_hip import lib
    todo = [tuple(r[:2]) for r in ROWS] + [tuple(r[:2]) for r in CHAIN_ROWS]
    if len(sys.argv) > 1 and sys.argv[1] == "all":              # every layer at more budgets: for extending the table
        todo = [(n, b) for n in LAYERS for b in (8, 16, 24, 32, 40, 48, 64)]
    for layer, budget in todo:
        assert lib.raw("avid_set_cu_budget")(budget) == budget
        print("ROW " + json.dumps([layer, budget] + list(names_now(layer))), flush=True)
    print("CUS %d" % lib.raw("avid_set_cu_budget")(0), flush=True)          # every CU: 256 without a GPU
    for layer in FULL:
        print("FULL " + json.dumps([layer] + list(names_now(layer)[:2])), flush=True)
