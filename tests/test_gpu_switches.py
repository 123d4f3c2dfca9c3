"""Every runtime switch of INTEGRATION.md ("Runtime switches") at its NON-default value: three engine steps on a fixed
small batch in a fresh process per setting (the switches are read once, at import or first use) against the default
run — bit-identical where only the arrangement changes (streams, launch programs, a one-rank process group), within fp32
summation-order noise where a different kernel / fusion computes the same numbers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _probe(env):
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(HERE, "_switch_probe.py")], env=e, capture_output=True, text=True,
                         timeout=600)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]
    assert out.returncode == 0 and line, (env, out.stdout[-800:], out.stderr[-1500:])
    return json.loads(line[-1][6:])


@pytest.fixture(scope="module")
def default_run(gpu_device):
    return _probe({})


IDENTICAL = [{"AVID_PLAN": "0"}, {"AVID_STEM_WGRAD_PRE": "0"},    # (dy split at commit time or per use: the same split, the same sums)
             {"AVID_WINO2_PRE": "0"},                             # (V split by the transform or by every product wave: likewise)
             {"AVID_WGRAD_PRE": "0"},                             # (grouped weight gradients: fragments split at the LDS write or per use)
             {"AVID_PK_WS": "0"},                                 # (K-split tails dealt tile-major or weight-stationary: same units, same slab order)
              {"AVID_OVERLAP_TOWERS": "0"}, {"AVID_DEFER_WGRAD": "0"}, {"AVID_STREAM_PROBE": "0"},
             {"AVID_FORCE_DIST": "1"}, {"AVID_FORCE_DIST": "1", "AVID_BUCKET_MB": "2"},
             {"AVID_HIP_LIB": os.path.join(os.path.dirname(HERE), "avid-cma_amd", "avid_hip", "libavid_hip.so")}]
CLOSE = [{"AVID_GROUP_WGRAD": "0"}, {"AVID_WGRAD_BF16X3": "0"}, {"AVID_FUSE_BN_BWD": "0"}, {"AVID_FUSE_BN_STATS": "0"}, {"AVID_FUSE_RES": "0"},
         {"AVID_FUSE_STEM_TAIL": "0"}, {"AVID_FUSED_CRITERION": "0"}, {"AVID_WINO": "0"}, {"AVID_WINO_WGRAD": "0"},
         {"AVID_TRIM_TAPS": "0"}, {"AVID_STEM_BF16X3": "0"}, {"AVID_STEM_FWD_PRE": "0"}, {"AVID_STEM_FWD_TM": "2"},
         # eight CUs (one per XCD) left to co-running kernels: other K-splits / slab counts, i.e. another summation order
         {"AVID_CU_RESERVE": "8"},
         # conv2x's temporal layers through tconv64_kernel / twgrad64_kernel at this small batch too (the default rule wants
         # three rounds of tiles), pre-split weights for every launch of the 128 x 128 tile, the criterion kernel's variants
         {"AVID_TCONV": "2"}, {"AVID_TCONV": "0"}, {"AVID_BS_WIDE": "1"}, {"AVID_BS_WIDE": "0"}, {"AVID_BS_ROWS": "0"},
         # every tail without full tiles weight-stationary, unsplit ones too: their BatchNorm partial rows change owners
         {"AVID_PK_WS": "2"},
         # the strided input gradients of the Cin % 128 == 0 layers on the 128 x 128 tile (both operands split in registers)
         {"AVID_S2_WIDE": "1"}]


@pytest.mark.parametrize("env", IDENTICAL, ids=lambda e: ",".join(f"{k}={v if len(v) < 9 else '...'}" for k, v in e.items()))
def test_arrangement_switches_are_bit_identical(default_run, env):
    got = _probe(env)
    assert got["losses"] == default_run["losses"]
    assert got["grad_sha"] == default_run["grad_sha"]


@pytest.mark.parametrize("env", CLOSE, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_kernel_switches_agree_to_summation_noise(default_run, env):
    _assert_close(_probe(env), default_run, env)


def _assert_close(got, default_run, env):
    # same weights at step 1; later steps drift apart: Adam's first updates are +-lr whatever the gradient's size, so a
    # gradient that differs in the last bits near zero (or one flipped ReLU / max-pool tie) moves a weight the other way
    for a, b, tol in zip(got["losses"], default_run["losses"], (3e-6, 2e-3, 1e-2)):
        assert abs(a - b) <= tol * abs(b), (got["losses"], default_run["losses"])
    np.testing.assert_allclose(got["grad_norm"], default_run["grad_norm"], rtol=1e-3)
    a, b = np.array(got["grad_probe"]), np.array(default_run["grad_probe"])
    # (a different convolution algorithm flips a few near-zero ReLU inputs / pooling near-ties; the gradients of the earliest
    #  layers see every one of them: per-layer parity is pinned in test_gpu_ops.py / test_gpu_model.py)
    #  (the stem's switch changes the roundings of the first layer, i.e. the input of every other one)
    #  (conv2x's temporal layers on another kernel: the same class — every later layer sees their roundings)
    #  (a CU budget changes the stem's grid, i.e. the order in which its BatchNorm partial sums are added: the statistics of the
    #   FIRST BatchNorm move in their last bits — the outputs themselves are bit-identical at any grid, tools/stem_grid_check.py)
    loose = ("AVID_WINO" in env or "AVID_STEM_BF16X3" in env or "AVID_TCONV" in env or "AVID_CU_RESERVE" in env or
             any(k.startswith("AVID_STEM_FWD") for k in env))
    assert np.abs(a - b).max() <= (3e-2 if loose else 1e-3) * np.abs(b).max() + 1e-7


def test_cu_budget_is_deterministic_and_reported(gpu_device):
    """A budget changes the persistent kernels' plans (tile deal, K-splits, slab counts), never the arithmetic: two runs at
    the same budget are bit-identical, and the library reports the CUs it plans for (a multiple of 8)."""
    a = _probe({"AVID_CU_RESERVE": "8"})
    b = _probe({"AVID_CU_RESERVE": "8"})
    assert a["losses"] == b["losses"] and a["grad_sha"] == b["grad_sha"]
    import torch
    from avid_hip import ops
    full = ops.cu_budget()
    try:
        assert ops.set_cu_budget(full - 8) == (full - 8) // 8 * 8
        assert ops.set_cu_budget(full - 3) == (full - 3) // 8 * 8
        assert ops.set_cu_budget(1) == 8
        assert ops.set_cu_budget(10 * full) == full
    finally:
        assert ops.set_cu_budget(0) == full == torch.cuda.get_device_properties(0).multi_processor_count


def test_arrangement_switches_stay_bit_identical_at_a_64_cu_budget(default_run, gpu_device):
    """Three bs-4 probes planning for 64 CUs (a quarter of the chip: whole rounds + K-split tails at this batch): alone, with
    the per-layer path instead of the launch programs, and with every K-split tail dealt tile-major.  Bit-identical among the
    three — launch programs == per-layer path and weight-stationary == tile-major order hold under a budget too — and the first
    within the CLOSE rule for AVID_CU_RESERVE of the default run."""
    import torch
    full = torch.cuda.get_device_properties(0).multi_processor_count
    if full <= 64:
        pytest.skip(f"a budget of 64 CUs is no reduction on a device of {full}")
    reserve = {"AVID_CU_RESERVE": str(full - 64)}
    alone = _probe(reserve)
    for extra in ({"AVID_PLAN": "0"}, {"AVID_PK_WS": "0"}):
        got = _probe({**reserve, **extra})
        assert got["losses"] == alone["losses"], extra
        assert got["grad_sha"] == alone["grad_sha"], extra
    _assert_close(alone, default_run, reserve)


def test_batchnorm_applied_by_its_consumer_is_bit_identical_at_batch_64(gpu_device):
    """AVID_IN_AFFINE: at the benchmark's batch conv2x's temporal layers (tconv64_kernel / twgrad64_kernel) apply the BatchNorm
    (+ReLU) in front of them while they stage its INPUT — fma(x, scale, shift), max(., 0): bn_apply_kernel's expression — and the
    four normalised tensors are never written.  Same values element for element, so three steps are bit-identical to the
    unfused arrangement (which the small-batch probes above run: tconv64_kernel wants three rounds of tiles)."""
    on = _probe({"PROBE_BS": "64"})
    off = _probe({"PROBE_BS": "64", "AVID_IN_AFFINE": "0"})
    assert on["losses"] == off["losses"] and on["grad_sha"] == off["grad_sha"]
