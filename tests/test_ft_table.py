"""Host checks (no GPU) behind tests/test_gpu_ft_layers.py: the layer tables of the two shipped fine-tuning shapes against
the launch programs compiled from the shipped wrapper, so that a model or planner change cannot alter what fine-tuning
launches without failing here, and the pinned-kernels file against the tables."""
import json
import os

import pytest

import _f64conv as R

KEYS = ["8x8x224", "4x32x224"]


def test_fixture_holds_the_two_shipped_shapes():
    from test_finetune_host import SHAPES
    tables = R.load_ft_tables()
    assert list(tables) == KEYS == list(R.FT_SHAPES)
    assert [tuple(tables[k]["video"]) for k in KEYS] == [R.FT_SHAPES[k] for k in KEYS] == SHAPES
    assert all(sorted(t) == ["groups", "layers", "model", "video"] and t["model"] == R.FT_MODEL for t in tables.values())


@pytest.mark.parametrize("key", KEYS)
def test_ft_layer_table_matches_the_programs(key):
    """The fixture is what the full-mode fine-tuning programs hold today: 21 distinct convolution geometries per shape (the
    stem at 224 x 224, 17 tower layers incl. the strided residual convolutions, and the three 1x1x1 residual entries that
    exist only as compact input gradients), none of them a geometry of the batch-64 table; three grouped weight-gradient
    launches.  At 8 frames conv2x's temporal layer takes the in-affine forms, at 32 frames the plain ones."""
    want = R.load_ft_tables()[key]
    got = R.trace_ft_table(R.FT_SHAPES[key])
    assert len(got["layers"]) == len(want["layers"]) == 21
    assert got == want
    ids = [R.layer_id(e) for e in got["layers"]]
    assert len(set(ids)) == 21 and not set(ids) & {R.layer_id(e) for e in R.load_bs64_table()["layers"]}
    assert all(e["fwd"] or e["dgrad"] for e in got["layers"])
    kinds = {w for e in got["layers"] for w in e["wgrad"]}
    in_affine = [e for e in got["layers"] if any(f[4] for f in e["fwd"])]
    only_dgrad = [e for e in got["layers"] if not e["fwd"] and not e["wgrad"]]
    assert len(only_dgrad) == 3 and all(e["k"] == [1, 1, 1] and e["dgrad"] == [[0, 0, 0, 0, 0]] for e in only_dgrad)
    assert sum(1 for e in got["layers"] if [1, 1, 2, 2, 2] in e["dgrad"]) == 3          # compact strided addends
    if key == "8x8x224":
        assert [len(g) for g in got["groups"]] == [12, 7, 5]
        assert kinds == {"own", "grouped", "in_affine"}
        assert [R.layer_id(e) for e in in_affine] == ["64to64_k311_s111_x8x56x56"]
        assert in_affine[0]["fwd"] == [[0, 1, 0, 0, 2], [1, 1, 0, 0, 2]] and in_affine[0]["wgrad"] == ["in_affine"]
    else:
        assert [len(g) for g in got["groups"]] == [10, 6, 5]
        assert kinds == {"own", "grouped"}
        assert not in_affine
        e = got["layers"][ids.index("64to64_k311_s111_x32x56x56")]
        assert e["fwd"] == [[0, 1, 0, 0, 0], [1, 1, 0, 0, 0]] and e["wgrad"] == ["own"]
    for g in got["groups"]:
        assert all("grouped" in got["layers"][i]["wgrad"] for i in g)


@pytest.mark.parametrize("key", KEYS)
def test_pinned_kernels_cover_every_direction_of_the_table(key):
    """tests/golden/ft_conv_kernels.json (the kernels that serve each direction, asserted by tests/test_gpu_ft_layers.py)
    names exactly the directions and forms of the layer table, each with at least one kernel."""
    with open(os.path.join(R.HERE, "golden", "ft_conv_kernels.json")) as f:
        pins = json.load(f)
    assert list(pins) == KEYS
    pinned, table = pins[key], R.load_ft_tables()[key]
    want = {}
    for e in table["layers"]:
        keys = ["fwd " + ",".join(map(str, f)) for f in e["fwd"] if not f[4]]      # (in-affine forms: pinned["in_affine"])
        keys += ["dgrad " + ",".join(map(str, f)) for f in e["dgrad"]]
        keys += ["wgrad"] if e["wgrad"] else []
        want[R.layer_id(e)] = sorted(keys)
    assert {k: sorted(v) for k, v in pinned["layers"].items()} == want
    assert all(ks for v in pinned["layers"].values() for ks in v.values())
    has_in_affine = any(f[4] for e in table["layers"] for f in e["fwd"])
    assert sorted(pinned["in_affine"]) == (["fwd", "wgrad"] if has_in_affine else []) and all(pinned["in_affine"].values())
    assert len(pinned["groups"]) == len(table["groups"]) and all(pinned["groups"])


def test_float32_yardstick_is_open_to_long_weight_gradients_only():
    """The entries test_gpu_ft_layers.py holds to 3x float32 instead of the rms bar are weight gradients over more output
    rows than any contraction the rms bar was set on (test_gpu_precision.CASES: 2 x 8 x 56 x 56 = 50 176)."""
    import test_gpu_ft_layers as FT
    tables = R.load_ft_tables()
    assert sorted(FT.FT_LONG_WGRAD) == sorted(KEYS)
    for key, names in FT.FT_LONG_WGRAD.items():
        by_id = {R.layer_id(e): e for e in tables[key]["layers"]}
        for name in names:
            assert by_id[name]["wgrad"] and FT.out_rows(by_id[name]) > FT.PRECISION_ROWS == 50176, (key, name)
