"""The recorded answers of the convolution queries: tests/golden/conv_routes.json.

Which kernel runs a layer, with which workspace and how many partial rows, is decided on the host from the descriptor, the CU
count and a handful of switches; Python compiles programs and sizes buffers from the answers.  The fixture holds, for a list
of (layer, batch) under every configuration of the switches, what every query answers for the forward (which 0), the input
gradient (1) and the weight gradient (2).  It is recorded ONCE, from the library of the commit named in its metadata, and
replayed string for string by tests/test_conv_routes_host.py: a mismatch is a change of behaviour, never a reason to record again.

    python tools/record_conv_routes.py --commit <hash of the commit whose library is loaded> [--out FILE]

No GPU is needed (without one the library plans for 256 CUs, the MI355X's count: ``meta.cus``); on a device with another
count only the configurations with a CU budget, whose plans do not depend on the device, are comparable.

Configurations.  The switches with a configure call are set in-process, one after the other (``INPROC``); the ones the library
reads once per process from the environment get a child process per non-default value (``ENV``); these and the CU budgets are
recorded at the batches ``ENV_BATCHES`` only.  ``collect(group)`` is what a child runs and what the test calls again.

Layout: ``entries[config][layer@B]`` = FIELDS in order; a configuration other than ``default`` holds only the layers whose
answers differ from ``default``'s (``expand`` puts the others back)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "conv_routes.json")
for _p in (REPO, os.path.join(REPO, "avid-cma_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIELDS = ("name0", "name1", "name2", "split0", "split1", "wino0", "wino1", "wino2", "ws_fwd", "ws_dgrad", "ws_wgrad",
          "fwd_stats_rows", "dgrad_bn_rows", "wgrad_groupable", "takes_in_affine", "takes_out_affine")
BATCHES = (1, 2, 8, 64)
ENV_BATCHES = (2, 64)
# (configuration, [(call, argument)]) applied on top of the defaults; undone before the next one
INPROC = (("default", []), ("tconv0", [("tconv", 0)]), ("tconv2", [("tconv", 2)]), ("wino0", [("wino", 0)]),
          ("cu8", [("cu", 8)]), ("cu16", [("cu", 16)]), ("cu24", [("cu", 24)]), ("cu40", [("cu", 40)]))
# one child process per value; TCONV_ENV also record under tconv 2, where the tconv64 / twgrad64 switches show
TCONV_ENV = ("AVID_IN_AFFINE=0", "AVID_TCONV_PARTS=7", "AVID_TCONV_PARTS=1")
ENV = ("AVID_S2_WIDE=1", "AVID_BS_WIDE=0", "AVID_BS_WIDE=1", "AVID_BS_ROWS=0", "AVID_PK_WS=0", "AVID_PK_WS=2",
       "AVID_TRIM_TAPS=0", "AVID_IN_AFFINE=0", "AVID_TCONV_PARTS=7", "AVID_TCONV_PARTS=1")
GROUPS = ("inproc",) + ENV


def conv_bench_layers():
    """The list ``L`` of tools/conv_bench.py, read from its source (the script itself runs the benchmark on import)."""
    import ast
    tree = ast.parse(open(os.path.join(REPO, "tools", "conv_bench.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "L":
            return ast.literal_eval(node.value)
    raise RuntimeError("tools/conv_bench.py: no list L")


def layers(batches=BATCHES):
    """[(id, (B, T, H, W), Cin, Cout, k, stride, pad, channel_first)]"""
    import _large_ref as G
    out = []
    for name, cin, cout, k, st, pd, thw in conv_bench_layers():
        for B in batches:
            out.append((f"{name}@{B}", (B,) + tuple(thw), cin, cout, tuple(k), tuple(st), tuple(pd), False))
    # both stems; two gather layers (channel-first, as every layer with Cin % 32 != 0 arrives: the input-gradient queries of a
    # channels-last one divide by zero in the recorded library); a refused stride; the strided layers at odd extents
    extra = {
        "video_stem": (3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3), (8, 32, 32), True),
        "audio_stem": (1, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), (1, 40, 100), True),
        "audio_gather": (1, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), (1, 50, 65), True),
        "gather16": (16, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (4, 14, 14), True),
        "stride3": (64, 64, (1, 3, 3), (1, 3, 3), (0, 1, 1), (4, 28, 28), False),
        "compact_122": (64, 128, (1, 1, 1), (1, 2, 2), (0, 0, 0), (7, 13, 15), False),
        "strided_222": (64, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1), (7, 13, 15), False),
        "temporal_13x15": (64, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), (8, 13, 15), False),
    }
    for name, (cin, cout, k, st, pd, thw, cf) in extra.items():
        for B in BATCHES[:2]:
            out.append((f"{name}@{B}", (B,) + thw, cin, cout, k, st, pd, cf))
    if batches is BATCHES:      # tests/_large_ref.py: the descriptors that cross 2 GiB / 4 GiB / 2^31 elements
        for name, B in G.CONV_2G + G.CONV_4G + [G.SPATIAL_2E31]:
            cin, cout, k, st, pd, thw, cf = G.LAYERS[name]
            out.append((f"large.{name}@{B}", (B,) + thw, cin, cout, k, st, pd, cf))
    return out


def query(d):
    """FIELDS of one descriptor.  A refused kernel name is recorded as "!<error code>"."""
    from avid_hip import lib
    ref = C.byref(d)
    buf = C.create_string_buffer(256)
    names = []
    for which in (0, 1, 2):
        rc = lib.raw("avid_conv_kernel_name")(ref, which, buf, 256)
        names.append(buf.value.decode() if rc == 0 else f"!{rc}")
    q = lambda fn, *a: int(lib.raw(fn)(ref, *a))   # noqa: E731
    return names + [q("avid_conv_uses_split", 0), q("avid_conv_uses_split", 1)] + \
        [q("avid_conv_uses_wino", w) for w in (0, 1, 2)] + \
        [q("avid_conv_fwd_workspace_bytes"), q("avid_conv_dgrad_workspace_bytes"), q("avid_conv_wgrad_workspace_bytes"),
         q("avid_conv_fwd_stats_rows"), q("avid_conv_dgrad_bn_rows"), q("avid_conv_wgrad_groupable"),
         q("avid_conv_takes_in_affine"), q("avid_conv_takes_out_affine")]


def _apply(settings):
    from avid_hip import lib
    cur = dict(tconv=-1, wino=-1, cu=0)
    cur.update(dict(settings))
    lib.raw("avid_tconv_configure")(cur["tconv"])
    lib.call("avid_wino_configure", cur["wino"], -1, -1)
    assert lib.raw("avid_set_cu_budget")(cur["cu"]) == (cur["cu"] or lib.raw("avid_cu_budget")())


def collect(group):
    """{configuration: {layer@B: FIELDS}} of one group, in THIS process: "inproc", or one of ENV (which must already be in the
    environment: the library reads it once).  Leaves the switches at their defaults."""
    from avid_hip import ops
    if group == "inproc":
        configs, ls = INPROC, None       # (every batch; the CU budgets at ENV_BATCHES, like the environment's switches)
    else:
        key, val = group.split("=")
        assert os.environ.get(key) == val, f"{group} must be set before the library is loaded"
        configs, ls = ((group, []),) + (((group + "+tconv2", [("tconv", 2)]),) if group in TCONV_ENV else ()), layers(ENV_BATCHES)
    out = {}
    try:
        for config, settings in configs:
            _apply(settings)
            rows = ls or layers(ENV_BATCHES if "cu" in dict(settings) else BATCHES)
            out[config] = {lid: query(ops._desc(shp, cin, cout, k, st, pd, cf)) for lid, shp, cin, cout, k, st, pd, cf in rows}
    finally:
        _apply([])
    return out


def expand(entries, config, ids):
    """The answers of ``config`` for the layers ``ids`` from the file's entries: its own where it holds one, else ``default``'s."""
    return {lid: entries[config].get(lid, entries["default"][lid]) for lid in ids}


def spawn(group, lib_path=None):
    """A child process that prints ``collect(group)`` as one JSON line."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AVID_")}
    if lib_path:
        env["AVID_HIP_LIB"] = lib_path
    if group != "inproc":
        key, val = group.split("=")
        env[key] = val
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", group], env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True)


def collect_all(lib_path=None):
    """Every group, each in a process of its own (the switches are process-global), side by side."""
    procs = [(g, spawn(g, lib_path)) for g in GROUPS]
    entries, cus, version = {}, None, None
    for g, p in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, (g, p.returncode, se[-1500:])
        got = json.loads(so.splitlines()[-1])
        entries.update(got["entries"])
        cus, version = got["cus"], got["version"]
    return entries, cus, version


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit whose library is loaded: goes into the metadata")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", help="print one group's answers as JSON (what collect_all starts)")
    ap.add_argument("--lib", help="the library to ask (default: the tree's)")
    a = ap.parse_args()
    if a.child:
        from avid_hip import lib
        print(json.dumps(dict(entries=collect(a.child), cus=int(lib.raw("avid_cu_budget")()), version=int(lib.version()))))
        return
    assert a.commit, "--commit is required"
    entries, cus, version = collect_all(a.lib)
    meta = dict(commit=a.commit, library_version=version, cus=cus, fields=FIELDS,
                note="recorded once from the library of `commit`; replayed by tests/test_conv_routes_host.py")
    lines = ["{", '"meta": ' + json.dumps(meta) + ",", '"entries": {']
    for ci, (config, rows) in enumerate(entries.items()):
        if config != "default":
            rows = {lid: v for lid, v in rows.items() if v != entries["default"][lid]}
        lines.append(json.dumps(config) + ": {")
        lines += [json.dumps(lid) + ": " + json.dumps(v, separators=(",", ":")) + ("," if i + 1 < len(rows) else "")
                  for i, (lid, v) in enumerate(rows.items())]
        lines.append("}" + ("," if ci + 1 < len(entries) else ""))
    lines += ["}", "}"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    size = os.path.getsize(a.out)
    assert size <= 1000 * 1000, f"{a.out}: {size} bytes"
    json.load(open(a.out))
    print(f"wrote {a.out}: {size} bytes, {len(entries)} configurations, {sum(len(r) for r in entries.values())} answers")


if __name__ == "__main__":
    main()
