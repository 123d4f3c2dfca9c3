"""Host checks (no GPU) behind tests/test_gpu_bs64_layers.py: the float64 convolution reference of tests/_f64conv.py against
float64 F.conv3d forward and backward, and the batch-64 layer table fixture against the launch programs compiled from the
model, so that a model or planner change cannot shrink the table silently."""
import pytest
import torch
import torch.nn.functional as F

import _f64conv as R

# name, Cin, Cout, k, stride, pad, (B,T,H,W)
CASES = [
    ("strided_padded", 3, 5, (1, 3, 3), (1, 2, 2), (0, 1, 1), (3, 2, 7, 9)),
    ("temporal_strided", 4, 6, (3, 1, 1), (2, 1, 1), (1, 0, 0), (2, 5, 3, 4)),
    ("stem_like", 2, 4, (3, 7, 7), (1, 2, 2), (1, 3, 3), (2, 3, 11, 10)),
    ("dead_taps_T1", 5, 3, (3, 1, 1), (1, 1, 1), (1, 0, 0), (4, 1, 3, 2)),
    ("one_by_one", 7, 4, (1, 1, 1), (1, 1, 1), (0, 0, 0), (3, 2, 3, 3)),
    ("one_by_one_s2", 4, 6, (1, 1, 1), (2, 2, 2), (0, 0, 0), (2, 5, 5, 6)),
]


@pytest.mark.parametrize("chunk", [1, 8])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_matches_conv3d(case, chunk):
    name, cin, cout, k, stride, pad, (B, Ti, Hi, Wi) = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, cin, Ti, Hi, Wi, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn((cout, cin) + k, generator=g, dtype=torch.float64).requires_grad_(True)
    y = F.conv3d(x, w, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    cl = lambda t: t.detach().permute(0, 2, 3, 4, 1).contiguous()           # noqa: E731
    got = R.conv_ref(cl(x), w.detach(), stride, pad, dy=cl(dy), chunk=chunk)
    torch.testing.assert_close(got["y"], cl(y), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got["dx"], cl(x.grad), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got["dw"], w.grad, rtol=1e-12, atol=1e-12)
    if name == "dead_taps_T1":
        assert bool((got["dw"][:, :, [0, 2]] == 0).all())                   # taps that only meet padding


def test_reference_calls_no_library_op():
    import inspect
    assert "avid_hip" not in inspect.getsource(R.conv_ref)


def test_bs64_layer_table_matches_the_model():
    """The fixture is what the batch-64 launch programs hold today: 32 distinct convolution geometries (video stem, audio
    stem, 9 audio / 19 video layers incl. the residual convolutions and their compact input gradients, the heads), each
    with its forward / input-gradient forms and weight-gradient kind, and the grouped weight-gradient launches."""
    want = R.load_bs64_table()
    got = R.trace_bs64_table()
    assert len(got["layers"]) == len(want["layers"]) == 32
    assert got == want
    kinds = {w for e in got["layers"] for w in e["wgrad"]}
    assert kinds == {"own", "grouped", "in_affine"}
    assert sum(1 for e in got["layers"] if any(f[4] for f in e["fwd"])) == 1      # conv2x's temporal layer
    assert [len(g) for g in got["groups"]] == [12, 7, 5, 9]


def test_pinned_kernels_cover_every_direction_of_the_table():
    """tests/golden/bs64_conv_kernels.json (the kernels that serve each direction at batch 64, asserted by
    tests/test_gpu_bs64_layers.py) names exactly the directions and forms of the layer table, each with at least one kernel."""
    import json
    import os
    with open(os.path.join(R.HERE, "golden", "bs64_conv_kernels.json")) as f:
        pinned = json.load(f)
    table = R.load_bs64_table()
    want = {}
    for e in table["layers"]:
        keys = ["fwd " + ",".join(map(str, f)) for f in e["fwd"] if not f[4]]      # (in-affine forms: pinned["in_affine"])
        keys += ["dgrad " + ",".join(map(str, f)) for f in e["dgrad"]]
        keys += ["wgrad"] if e["wgrad"] else []
        want[R.layer_id(e)] = sorted(keys)
    assert {k: sorted(v) for k, v in pinned["layers"].items()} == want
    assert all(ks for v in pinned["layers"].values() for ks in v.values())
    assert sorted(pinned["in_affine"]) == ["fwd", "wgrad"] and all(pinned["in_affine"].values())
    assert len(pinned["groups"]) == len(table["groups"]) and all(pinned["groups"])


# ---- BatchNorm reference and the table of the step's other launches -------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", [(2, 3), (37, 8), (1000, 5)])
def test_bn_reference_matches_batch_norm(M, C, relu):
    """tests/_f64conv.bn_ref against float64 F.batch_norm (training mode, momentum 0.1): saved mean / invstd, y, running
    statistics, dx, dgamma, dbeta to 1e-12."""
    g = torch.Generator().manual_seed(M * 10 + C)
    x = (torch.randn(M, C, generator=g, dtype=torch.float64) * 1.7 + 0.3).requires_grad_(True)
    gamma = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5 + 1.0).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    rm_t, rv_t = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm_t, rv_t, gamma, beta, True, 0.1, 1e-5)
    if relu:
        y = F.relu(y)
    (y * dy).sum().backward()
    got = R.bn_ref(x.detach(), gamma.detach(), beta.detach(), rm, rv, 0.1, 1e-5, relu=relu, dy=dy)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)      # noqa: E731
    close(got["y"], y.detach())
    close(got["running_mean"], rm_t)
    close(got["running_var"], rv_t)
    close(got["dx"], x.grad)
    close(got["dgamma"], gamma.grad)
    close(got["dbeta"], beta.grad)
    xd = x.detach()
    close(got["mean"], xd.mean(0))
    close(got["invstd"], 1.0 / torch.sqrt(xd.var(0, unbiased=False) + 1e-5))
    close(got["scale"] * xd + got["shift"], F.batch_norm(xd, None, None, gamma.detach(), beta.detach(), True, 0.1, 1e-5))


def test_bn_reference_calls_no_library_op():
    import inspect
    assert "avid_hip" not in inspect.getsource(R.bn_ref)


def test_bs64_norm_table_matches_the_programs():
    """The fixture is what the batch-64 launch programs hold today: 41 BatchNorm forwards and 41 backwards (16 / 21 distinct
    geometries and forms), the stem's BatchNorm + max-pool, two global pools each way, 4 ReLU backwards and 6 bias sums of the
    heads; the flat Adam buffer of 21 286 784 elements split at 21 258 432."""
    want = R.load_bs64_norm_table()
    got = R.trace_bs64_norm_table()
    assert got == want
    ops = got["ops"]
    counts = {k: sum(e["count"] for e in v) for k, v in ops.items()}
    assert counts == {"bn_fwd": 41, "bn_bwd": 41, "bn_pool_fwd": 1, "bn_pool_bwd": 1, "gpool_fwd": 2, "gpool_bwd": 2,
                      "relu_bwd": 4, "colsum": 6}
    assert len({(e["M"], e["C"], e["nparts"], e["relu"], e["y"]) for e in ops["bn_fwd"]}) == 16
    assert len({(e["M"], e["C"], e["nparts"], e["relu"], e["frozen"]) for e in ops["bn_bwd"]}) == 21
    assert sorted((e["S"], e["C"]) for e in ops["gpool_fwd"]) == [(16, 512), (21, 512)]
    assert sorted((e["M"], e["C"], e["count"]) for e in ops["colsum"]) == [(64, 128, 2), (64, 512, 4)]
    assert ops["relu_bwd"] == [{"n": 32768, "count": 4}]
    assert got["adam"] == {"n": 21286784, "early": 21258432}
    assert max(e["nparts"] for e in ops["bn_fwd"]) == 1536 and max(e["M"] for e in ops["bn_fwd"]) == 401408
    assert sum(e["count"] for e in ops["bn_fwd"] if not e["y"]) == 4                 # conv2x's deferred BatchNorms
    assert all(e["running"] and e["momentum"] == 0.1 for e in ops["bn_fwd"] + ops["bn_pool_fwd"])
    assert not any(e["frozen"] for e in ops["bn_bwd"])


def test_bs64_norm_table_partials_come_from_conv_epilogues():
    """Every BatchNorm record with partial rows names a convolution-table entry whose form makes them: a forward form with
    BatchNorm sums (the layer offers that many rows), or an input-gradient form with the fused BatchNorm-backward sums; the
    ones without come from a global pool; every backward reads a forward of its own geometry."""
    import json
    from avid_hip import ops as O
    table = R.load_bs64_norm_table()
    layers = R.load_bs64_table()["layers"]

    def desc(le):
        return O._desc_cached(tuple(le["x"]), le["Cin"], le["Cout"], tuple(le["k"]), tuple(le["stride"]), tuple(le["pad"]),
                              le["channel_first"])
    for e in table["ops"]["bn_fwd"] + table["ops"]["bn_pool_fwd"]:
        assert e["nparts"] > 0 and e["producer"] is not None
        le = layers[e["producer"]["conv"]]
        form = e["producer"]["fwd"]
        assert form in le["fwd"] and form[1] == 1, json.dumps(e)
        B, To = le["x"][0], R.out_size(le["x"][1], le["k"][0], le["stride"][0], le["pad"][0])
        Ho = R.out_size(le["x"][2], le["k"][1], le["stride"][1], le["pad"][1])
        Wo = R.out_size(le["x"][3], le["k"][2], le["stride"][2], le["pad"][2])
        M = e["M"] if "M" in e else e["B"] * e["T"] * e["H"] * e["W"]
        assert (B * To * Ho * Wo, le["Cout"]) == (M, e["C"])
        assert desc(le)[4] == e["nparts"]
    for e in table["ops"]["bn_bwd"]:
        fe = table["ops"]["bn_fwd"][e["fwd"]]
        assert (fe["M"], fe["C"], fe["relu"]) == (e["M"], e["C"], e["relu"])
        if e["producer"] is None:
            assert e["nparts"] == 0 and e["dy"] == "gpool_bwd" and fe["y"]
            continue
        le = layers[e["producer"]["conv"]]
        form = e["producer"]["dgrad"]
        assert form in le["dgrad"] and form[0] == 1, json.dumps(e)
        assert (le["x"][0] * le["x"][1] * le["x"][2] * le["x"][3], le["Cin"]) == (e["M"], e["C"])
        assert desc(le)[0].bn_bwd_rows == e["nparts"]
