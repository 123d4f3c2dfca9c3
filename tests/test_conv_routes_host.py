"""The convolution queries against their recorded answers (tests/golden/conv_routes.json, tools/record_conv_routes.py): kernel
name, pre-split / Winograd use, the three workspace sizes, BatchNorm partial rows, groupable, in- / out-affine — for every
recorded (layer, batch) under every configuration of the dispatch switches, every field equal, string for string.

No GPU is needed: without one the library plans for 256 CUs.  The switches are process-global or read once from the
environment: the library is asked in child processes (tools/record_conv_routes.py collect_all), all started side by side."""
import functools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import record_conv_routes as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "conv_routes.json")
PARENT = "266c4bd"      # the commit in front of the one that introduced conv_route: the file is its answers


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _now():
    return R.collect_all()


def test_the_file_is_the_parents_and_covers_every_configuration():
    g = _golden()
    assert g["meta"]["commit"].startswith(PARENT) and g["meta"]["cus"] == 256
    assert tuple(g["meta"]["fields"]) == R.FIELDS
    want = {c for c, _ in R.INPROC} | set(R.ENV) | {e + "+tconv2" for e in R.TCONV_ENV}
    assert set(g["entries"]) == want
    ids = [lid for lid, *_ in R.layers()]
    assert set(g["entries"]["default"]) == set(ids) and len(ids) == len(set(ids))
    for config, rows in g["entries"].items():          # (the others hold what differs from the default: R.expand)
        assert set(rows) <= set(ids) and (config == "default" or all(v != g["entries"]["default"][lid] for lid, v in rows.items()))
    # the families the recorded names must reach
    names = {n.split(" ")[0].split("<")[0] for rows in g["entries"].values() for v in rows.values() for n in v[:3]}
    for fam in ("stem_fwd3p_kernel", "igemm_gather_kernel", "wino_kernel", "tconv64_kernel", "twgrad64_kernel", "igemm_pk_kernel",
                "igemm_kernel", "stem_dgrad_kernel", "stem_wgrad_kernel", "wino_wgrad_kernel", "wgrad_tab_kernel", "wgrad_gather_kernel"):
        assert fam in names, (fam, sorted(names))


def test_every_query_answers_what_was_recorded():
    g = _golden()
    got, cus, _ = _now()
    assert set(got) == set(g["entries"])
    bad = []
    for config, rows in g["entries"].items():
        # (a plan for a budget below the CU count does not depend on the device; the others are the 256-CU plans)
        if cus != 256 and "cu" not in config:
            continue
        for lid, want in R.expand(g["entries"], config, got[config]).items():
            for field, a, b in zip(R.FIELDS, got[config][lid], want):
                if a != b:
                    bad.append(f"{config} {lid} {field}: {a!r}, recorded {b!r}")
    assert not bad, f"{len(bad)} answers differ:\n" + "\n".join(bad[:40])
