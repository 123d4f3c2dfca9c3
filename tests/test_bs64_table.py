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
