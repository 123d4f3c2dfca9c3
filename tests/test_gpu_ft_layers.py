"""Every convolution launch of the fine-tuning programs against float64, at the two shipped per-GPU clip shapes
(8 x 3x8x224x224 and 4 x 3x32x224x224) and under the default dispatch.

The layer tables (tests/golden/ft_conv_layers.json, checked against the compiled programs by tests/test_ft_table.py) list
the 21 distinct geometries of each shape and what the programs fuse into each.  Every entry runs through the checks of
tests/test_gpu_bs64_layers.py (its ``check_layer`` / ``check_in_affine`` / ``check_group``: the same C entry points and
arguments, every output pre-filled with NaN, the same float64 reference, the same bars — max|err| / max|ref| below 2e-5 for
outputs and input gradients, 5e-5 for weight gradients, partial sums within 1e-5 of the largest column's sum of |terms|,
rms(err) / rms(ref) <= 6e-7 for every direction served only by six-bf16-product kernels):
  * forward in every epilogue form, input gradient in every form (the three 1x1x1 residual entries exist only as input
    gradients), weight gradient on its own;
  * the in-affine forms of conv2x's temporal layer at 8 frames (at 32 frames the programs use the plain forms);
  * the six grouped weight-gradient launches with the programs' own members;
  * per shape, one real FinetuneStep step launches exactly the convolution-family kernels the pins imply.
A 32-frame clip is sixteen batch-64 clips, so the float64 reference goes one clip at a time there (two at 8 frames).

Which kernels serve each direction is pinned per entry (tests/golden/ft_conv_kernels.json, recorded on an MI355X under the
default dispatch in a run where the entry's float64 checks passed).  ``pytest -s`` prints every error next to its bar."""
import json
import os

import pytest
import torch

import _f64conv as R
import test_gpu_bs64_layers as CL
from test_gpu_bs64_layers import _default_dispatch  # noqa: F401  (autouse here too: the default dispatch is what runs)

pytestmark = pytest.mark.gpu

TABLES = R.load_ft_tables()
with open(os.path.join(R.HERE, "golden", "ft_conv_kernels.json")) as _f:
    KERNELS = json.load(_f)
CHUNK = {"8x8x224": 2, "4x32x224": 1}
# The longest contraction RMS_BAR was set on (test_gpu_precision.CASES: the stem at 2 x 8 x 56 x 56 output rows).
PRECISION_ROWS = 50176
# Weight gradients of six-product kernels over more than PRECISION_ROWS output rows whose rms error against float64 is above
# RMS_BAR: held, as test_gpu_bs64_layers.LONG_WGRAD is, to 3x the rms error of the same contraction in plain float32
# (tests/_f64conv.py, dtype=float32).  Measured on an MI355X, rms(err)/rms(ref) of the kernel, then of float32:
#   8 frames:  stem, stem_wgrad3_kernel<3,3>, 0.8 M rows:                        2.5e-6 vs 4.1e-6 (0.62x)
#   32 frames: stem, stem_wgrad3_kernel<3,3>, 1.6 M rows:                        5.1e-6 vs 5.3e-6 (0.96x)
#              conv2x temporal, wgrad_tab_kernel<1,3>, 401 k rows:               1.0e-6 vs 3.4e-6 (0.30x)
#              conv3x.0 strided spatial, wgrad_tab_kernel<2,2>, 100 k rows:      7.1e-7 vs 1.8e-6 (0.40x)
# (none is less accurate than float32 itself).  Every other direction of both tables meets RMS_BAR, conv2x's temporal layer
# at 8 frames (twgrad64_kernel, 200 k rows) included: 5.8e-7 plain, 5.4e-7 / 5.7e-7 in-affine with ReLU / linear, against
# 2.4e-6, 1.8e-6 and 2.4e-6 in float32.
FT_LONG_WGRAD = {"8x8x224": ("3to64_k377_s122_x8x224x224_cf",),
                 "4x32x224": ("3to64_k377_s122_x32x224x224_cf", "64to64_k311_s111_x32x56x56", "64to128_k133_s122_x32x56x56")}

CASES = [(key, i) for key in TABLES for i in range(len(TABLES[key]["layers"]))]
GROUPS = [(key, gi) for key in TABLES for gi in range(len(TABLES[key]["groups"]))]


def out_rows(e):
    n = e["x"][0]
    for size, k, s, p in zip(e["x"][1:], e["k"], e["stride"], e["pad"]):
        n *= R.out_size(size, k, s, p)
    return n


@pytest.mark.parametrize("key,idx", CASES, ids=[f"{k}-{R.layer_id(TABLES[k]['layers'][i])}" for k, i in CASES])
def test_layer_against_float64(key, idx, gpu_device, kernel_log):
    CL.check_layer(TABLES[key]["layers"][idx], idx, KERNELS[key], gpu_device, kernel_log, long_wgrad=FT_LONG_WGRAD[key],
                   chunk=CHUNK[key])


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_conv2x_temporal_layer_in_the_programs_form(relu, gpu_device, kernel_log):
    """conv2x's temporal layer as the 8-frame programs run it (avid_conv_fwd_in / avid_conv_wgrad_in), checked as
    test_gpu_bs64_layers.test_conv2x_temporal_layer_in_the_programs_form checks it at 64 clips; the 32-frame programs hold
    no in-affine form."""
    assert not any(f[4] for e in TABLES["4x32x224"]["layers"] for f in e["fwd"])
    e = CL._conv2x_temporal(TABLES["8x8x224"]["layers"])
    assert e["x"] == [8, 8, 56, 56] and e["k"] == [3, 1, 1] and e["wgrad"] == ["in_affine"]
    CL.check_in_affine(e, relu, KERNELS["8x8x224"], gpu_device, kernel_log, long_wgrad=FT_LONG_WGRAD["8x8x224"],
                       chunk=CHUNK["8x8x224"])


@pytest.mark.parametrize("key,gi", GROUPS, ids=[f"{k}-group{gi}" for k, gi in GROUPS])
def test_grouped_weight_gradients_of_the_programs(key, gi, gpu_device, kernel_log):
    CL.check_group(TABLES[key], gi, KERNELS[key], gpu_device, kernel_log, chunk=CHUNK[key])


def implied_kernels(table, pins):
    """The convolution-family kernels a step launches if every launch of the table is served as pinned: each forward and
    input-gradient form, a weight gradient of its own only where the programs launch one, the in-affine forms, the groups."""
    ks = set()
    for e in table["layers"]:
        p = pins["layers"][R.layer_id(e)]
        for f in e["fwd"]:
            ks |= set(pins["in_affine"]["fwd"] if f[4] else p[CL._form_key("fwd", f)])
        for f in e["dgrad"]:
            ks |= set(p[CL._form_key("dgrad", f)])
        if "own" in e["wgrad"]:
            ks |= set(p["wgrad"])
        if "in_affine" in e["wgrad"]:
            ks |= set(pins["in_affine"]["wgrad"])
    for g in pins["groups"]:
        ks |= set(g)
    return ks


@pytest.mark.parametrize("key", list(TABLES))
def test_step_launches_exactly_the_pinned_kernels(key, gpu_device, kernel_log):
    """One real FinetuneStep step of the shipped wrapper at the shipped shape launches exactly the convolution-family
    kernels the table and its pins imply: no launch of the step escapes the float64 checks above."""
    import models
    from avid_hip.parallel import FinetuneStep
    dev = gpu_device
    shape = R.FT_SHAPES[key]
    assert TABLES[key]["video"] == list(shape)
    torch.manual_seed(0)
    model = models.ClassificationWrapper(models.R2Plus1D(18), 101, feat_name="pool", feat_dim=512, pooling_op=None,
                                         use_dropout=True, dropout=0.5).to(dev).train()
    eng = FinetuneStep(model)
    g = torch.Generator().manual_seed(1234)
    video = torch.randn(*shape, generator=g).to(dev)
    labels = torch.randint(0, 101, (shape[0],), generator=g).to(dev)
    eng.step(video, labels)                        # (compiles the programs, builds the weight tables)
    with kernel_log() as log:
        eng.step(video, labels)
    step = set(CL.conv_names(log.report))
    want = implied_kernels(TABLES[key], KERNELS[key])
    print(f"\n{key} step:", sorted(step), "\npinned:", sorted(want))
    assert step, "the step's launch log holds no convolution kernel"
    assert step == want, (sorted(step - want), sorted(want - step))
