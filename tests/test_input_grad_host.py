"""The bars of tests/test_gpu_input_grad.py can fail, and a correct float32 implementation clears them with room (no GPU).

At every shape of the GPU test: float32 torch on the CPU is inside the per-element bound of tests/_input_grad_ref.py (a
ceiling); a kernel that drops a tap, and one that drops a single weight, are at least 5 x outside it and at least 1000 x
float32's relative rms error (floors).  The float64 restatements of the towers are pinned to the modules they restate."""
import pytest
import torch

import _input_grad_ref as R


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_float32_is_inside_the_bound_and_the_mutants_are_not(shape):
    c = R.case(shape)
    assert c["dx64"].shape == c["xs"] and c["K"] == 64 * c["k"][0] * 16
    ratio32 = R.bound_ratio(c["dx32"], c)
    print(f"{R.shape_id(shape)}: float32 torch at {ratio32:.2e} of the bound, relative rms {c['rms32']:.2e}")
    assert ratio32 <= 1.0
    assert 0.0 < c["rms32"] < 1e-6
    for name, dx in R.mutants(c).items():
        ratio, rms = R.bound_ratio(dx, c), R.rel_rms(dx, c["dx64"])
        print(f"  {name}: {ratio:.1f} x the bound, relative rms {rms:.2e}")
        assert ratio >= 5.0, (name, ratio)
        assert rms >= 1000.0 * c["rms32"], (name, rms, c["rms32"])


def test_the_bound_is_the_first_order_bound_of_any_summation_order():
    """Summing the products of one element in float32 in reversed and in random order stays inside the bound too."""
    c = R.case((1, 3, 1, 7, 9))
    xs, pad = c["xs"], c["pad"]
    g = torch.Generator().manual_seed(7)
    for perm in (torch.arange(63, -1, -1), torch.randperm(64, generator=g)):
        acc = torch.zeros(xs)
        for co in perm.tolist():                 # one output channel at a time: another order of the same float32 sum
            acc = acc + R.dgrad(c["dy"][:, co:co + 1], c["w"][co:co + 1], xs, pad)
        assert R.bound_ratio(acc, c) <= 1.0


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_video_restatement_matches_the_reference_formulas(train):
    """``video_tower`` against torch.nn modules assembled as models.R2Plus1D(10) is (Conv3d / BatchNorm3d / ReLU / MaxPool3d),
    float64, same parameters: the restatement is the network the GPU test compares against."""
    import torch.nn as nn
    torch.manual_seed(3)
    sd = {}

    def conv(name, cin, cout, k, s, p):
        m = nn.Conv3d(cin, cout, k, s, p, bias=False).double()
        sd[name + ".weight"] = m.weight.detach()
        return m

    def bn(name, c):
        m = nn.BatchNorm3d(c).double()
        with torch.no_grad():
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.3, 0.3)
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 1.5)
        for k in ("weight", "bias", "running_mean", "running_var"):
            sd[f"{name}.{k}"] = getattr(m, k).detach().clone()
        return m.train(train)

    stem = nn.Sequential(conv("conv1.0", 3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3)), bn("conv1.1", 64), nn.ReLU(),
                         nn.MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1)))
    n = "conv2x"
    blk = [conv(n + ".spt_conv1", 64, 64, (1, 3, 3), 1, (0, 1, 1)), bn(n + ".spt_bn1", 64),
           conv(n + ".tmp_conv1", 64, 64, (3, 1, 1), 1, (1, 0, 0)), bn(n + ".tmp_bn1", 64),
           conv(n + ".spt_conv2", 64, 64, (1, 3, 3), 1, (0, 1, 1)), bn(n + ".spt_bn2", 64),
           conv(n + ".tmp_conv2", 64, 64, (3, 1, 1), 1, (1, 0, 0)), bn(n + ".out_bn", 64)]
    x = torch.randn(2, 3, 3, 16, 16, dtype=torch.float64)
    h0 = stem(x)
    h = h0
    for k in range(0, 6, 2):
        h = torch.relu(blk[k + 1](blk[k](h)))
    want = torch.relu(blk[7](blk[6](h) + h0)).amax(dim=(2, 3, 4), keepdim=True)
    got = R.video_tower(x, sd, train, stages=("conv2x",))
    assert got.shape == (2, 64, 1, 1, 1)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
