"""The step guard without a GPU: the engines' argument checks, the C ABI's refusals (nothing is launched), and the error bound
of ``grad_norm`` — a numpy emulation of the kernel's summation (tests/_guard_ref.py: same partition, same order, same number
formats) against the exactly rounded float64 sum, with three planted bugs that must land at least 10 x outside the bound."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _guard_ref as R

BADARG = -1                      # include/avid_hip.h: AVID_E_BADARG


def _tiny_model():
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.BatchNorm1d(8), torch.nn.Linear(8, 3))


class _Probe(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.feature_extractor = torch.nn.Linear(6, 6).requires_grad_(False)
        self.classifiers = torch.nn.ModuleList([torch.nn.Linear(6, 3), torch.nn.Linear(6, 3)])


def _engines():
    from avid_hip import parallel
    return ((parallel.TrainStep, _tiny_model, dict(criterion=None)), (parallel.FinetuneStep, _tiny_model, {}),
            (parallel.ProbeStep, _Probe, {}))


def test_version_and_record_layout():
    from avid_hip import lib
    assert lib.version() >= 164
    assert C.sizeof(lib.StepGuard) == 32
    offs = {n: getattr(lib.StepGuard, n).offset for n, _ in lib.StepGuard._fields_}
    assert offs == {"grad_norm": 0, "clip_coef": 4, "skip": 8, "reserved": 12, "skipped_total": 16, "steps_total": 24}
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avid_hip.h")).read()
    body = re.search(r"typedef struct avid_step_guard \{(.*?)\} avid_step_guard;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("float", "grad_norm"), ("float", "clip_coef"), ("int32_t", "skip"),
                                                    ("int32_t", "reserved"), ("int64_t", "skipped_total"),
                                                    ("int64_t", "steps_total")]


@pytest.mark.parametrize("bad", [0, -1, float("nan"), float("inf")])
def test_max_grad_norm_must_be_positive_and_finite(bad):
    for cls, model, kw in _engines():
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls(model(), max_grad_norm=bad, **kw)


def test_options_are_accepted_and_off_by_default():
    for cls, model, kw in _engines():
        plain = cls(model(), **kw)
        assert plain.guard is None and plain.max_grad_norm is None and plain.skip_nonfinite is False
        for opts in (dict(max_grad_norm=2.5), dict(skip_nonfinite=True), dict(max_grad_norm=1, skip_nonfinite=True)):
            eng = cls(model(), optimizer="sgd", momentum=0.9, **opts, **kw)
            g = eng.guard
            assert g is not None and g.record.numel() * g.record.element_size() == 32
            for name, dt in (("grad_norm", torch.float32), ("clip_coef", torch.float32), ("skipped", torch.int32),
                             ("skipped_total", torch.int64), ("steps_total", torch.int64)):
                view = getattr(g, name)
                assert view.dim() == 0 and view.dtype == dt and int(view) == 0
            g.record[2] = 1                                               # the views alias the record
            g.record.view(torch.int64)[3] = 7
            assert int(g.skipped) == 1 and int(g.steps_total) == 7
            assert eng.max_grad_norm == opts.get("max_grad_norm") and eng.skip_nonfinite == opts.get("skip_nonfinite", False)


def test_ops_refuse_cpu_tensors():
    from avid_hip import ops, AvidHipError
    guard = ops.StepGuard(torch.device("cpu"))
    z = torch.zeros(8)
    with pytest.raises(AvidHipError):
        ops.grad_guard(z, guard)
    with pytest.raises(AvidHipError):
        ops.adam_flat_guarded(z, z, z, z, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, guard)
    with pytest.raises(AvidHipError):
        ops.sgd_flat_guarded(z, z, None, 1e-3, 0.0, 0.0, guard)
    with pytest.raises(AvidHipError):
        ops.guard_restore(z, None, z, guard)
    with pytest.raises(AvidHipError):
        ops.guard_nonfinite(z, guard)


def test_entry_points_refuse_bad_arguments_before_launching():
    """n <= 0, null pointers, a short workspace: AVID_E_BADARG and a message, and no launch (there is no GPU here)."""
    from avid_hip import lib
    buf = (C.c_double * 64)()
    a = C.addressof(buf)                      # 16-byte aligned host memory: never dereferenced by a refused call
    a -= a % 16
    a += 16
    ws_bytes = lib.raw("avid_grad_guard_workspace_bytes")
    assert ws_bytes(0) == 0 and ws_bytes(-3) == 0
    assert ws_bytes(1) == 8 and ws_bytes(1024) == 8 and ws_bytes(1025) == 16
    assert ws_bytes(R.GRID_STRIDE) == ws_bytes(1 << 40) == 8 * R.MAX_BLOCKS
    for n in (1, 1024, 1025, 5000, R.GRID_STRIDE + 5):
        assert ws_bytes(n) == 8 * R.blocks_of(n)
    gg = lib.raw("avid_grad_guard")
    for args in ((0, a, 1.0, 0.0, 1, a, a, 1 << 20, None), (-4, a, 1.0, 0.0, 1, a, a, 1 << 20, None),
                 (8, None, 1.0, 0.0, 1, a, a, 1 << 20, None), (8, a, 1.0, 0.0, 1, None, a, 1 << 20, None),
                 (8, a, 1.0, 0.0, 1, a, None, 1 << 20, None), (8, a, 1.0, 0.0, 1, a, a, 7, None),
                 (5000, a, 1.0, 0.0, 1, a, a, 8 * R.blocks_of(5000) - 1, None), (8, a + 2, 1.0, 0.0, 1, a, a, 1 << 20, None)):
        assert gg(*args) == BADARG, args
        assert "grad_guard" in lib.last_error()
    adam = lib.raw("avid_adam_flat_guarded")
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    for args in ((0, a, a, a, a) + hyper + (1, None, None, 1.0, a, None), (8, None, a, a, a) + hyper + (1, None, None, 1.0, a, None),
                 (8, a, None, a, a) + hyper + (1, None, None, 1.0, a, None), (8, a, a, None, a) + hyper + (1, None, None, 1.0, a, None),
                 (8, a, a, a, None) + hyper + (1, None, None, 1.0, a, None), (8, a, a, a, a) + hyper + (1, None, None, 1.0, None, None),
                 (8, a, a, a, a) + hyper + (0, None, None, 1.0, a, None), (8, a + 4, a, a, a) + hyper + (1, None, None, 1.0, a, None)):
        assert adam(*args) == BADARG, args
        assert "adam_flat_guarded" in lib.last_error()
    sgd = lib.raw("avid_sgd_flat_guarded")
    for args in ((0, a, a, a, 0.1, 0.9, 0.0, 0, None, 1.0, a, None), (8, None, a, a, 0.1, 0.9, 0.0, 0, None, 1.0, a, None),
                 (8, a, None, a, 0.1, 0.9, 0.0, 0, None, 1.0, a, None), (8, a, a, None, 0.1, 0.9, 0.0, 0, None, 1.0, a, None),
                 (8, a, a, a, 0.1, 0.9, 0.0, 0, None, 1.0, None, None), (8, a, a, None, 0.1, 0.0, 0.0, 1, None, 1.0, a, None),
                 (8, a, a + 4, a, 0.1, 0.9, 0.0, 0, None, 1.0, a, None)):
        assert sgd(*args) == BADARG, args
        assert "sgd_flat_guarded" in lib.last_error()
    unless = lib.raw("avid_counter_add_unless")
    assert unless(None, 1, a, None) == BADARG and unless(a, 1, None, None) == BADARG
    witness = lib.raw("avid_guard_nonfinite")
    for args in ((0, a, a, None), (8, None, a, None), (8, a, None, None), (8, a + 2, a, None)):
        assert witness(*args) == BADARG, args
        assert "guard_nonfinite" in lib.last_error()
    restore = lib.raw("avid_guard_restore")
    for args in ((0, 4, a, None, a, a, None), (4, 0, a, None, a, a, None), (4, 4, None, None, a, a, None),
                 (4, 4, a, None, None, a, None), (4, 4, a, None, a, None, None)):
        assert restore(*args) == BADARG, args
        assert "guard_restore" in lib.last_error()


def _inputs(n, seed):
    """|g| in [0.5, 1.5): no element, and no 64 of them, is small against the whole — a dropped one shows."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], n) * (0.5 + rng.random(n))).astype(np.float32)


SIZES = (1, 3, 255, 256, 257, 1023, 4097, 70001, R.GRID_STRIDE + 1029)


@pytest.mark.parametrize("n", SIZES)
def test_kernel_summation_stays_inside_the_derived_bound(n):
    scale = 0.5
    for start in range(4):
        g = _inputs(n, 100 + start)
        want = R.guard_ref(g, scale)["norm"]
        got = R.kernel_norm(g, scale, start)
        err = abs(got - want) / want
        print(f"\n[guard bound] n {n} start {start}: emulation {got!r}, float64 {want!r}, rel {err:.3e}, bound {R.norm_bound(n):.3e}")
        assert err <= R.norm_bound(n), (n, start, err)
        head, n4, tail = R.partition(n, start)
        assert head + 4 * n4 + tail == n and 0 <= head < 4 and 0 <= tail < 4 and (head == n or (start + head) % 4 == 0)


def test_bound_is_what_design_derives():
    """2^-24 for the one fp32 rounding, plus (k / 2 + 3) 2^-53 for the double chain: k = 47 additions at the model's
    21.3 M elements (21 grid-stride rounds), so the fp32 rounding is all of it to nine digits."""
    n = 21_300_000
    assert R.blocks_of(n) == 1024 and R.chain_length(n) == 21 + 1 + 2 + 6 + 3 + 4 + 6 + 3
    assert R.norm_bound(n) == 2.0 ** -24 + (46 / 2 + 3) * 2.0 ** -53
    assert R.norm_bound(n) < 2.0 ** -24 * (1 + 1e-7)


@pytest.mark.parametrize("n,start", [(4099, 0), (4098, 1), (70001, 2)])
def test_planted_bugs_land_ten_times_outside_the_bound(n, start):
    """Sizes at which one element of |g| >= 0.5 is still >= 10 bounds of the norm: about 1 / (2.2 n) against 6e-8."""
    scale = 0.5
    g = _inputs(n, 7)
    head, n4, tail = R.partition(n, start)
    assert tail >= 1 and n4 >= 32
    want = R.guard_ref(g, scale)["norm"]
    bound = R.norm_bound(n)
    for bug in (dict(drop_tail=True), dict(drop_slice=True), dict(scale_twice=True)):
        err = abs(R.kernel_norm(g, scale, start, **bug) - want) / want
        print(f"\n[guard bound] n {n} start {start} {bug}: rel {err:.3e} = {err / bound:.1f} x bound")
        assert err >= 10 * bound, (bug, err, bound)


def test_reference_judges_the_sum_as_fp32():
    g = _inputs(64, 3)
    assert R.guard_ref(g)["skip"] == 0 and R.guard_ref(g, max_norm=1e30)["coef"] == 1.0
    for poison in (float("nan"), float("inf"), -float("inf"), 3e19):
        h = g.copy()
        h[17] = poison
        r = R.guard_ref(h, max_norm=1.0)
        assert r["skip"] == 1 and r["coef"] == 1.0 and not math.isfinite(r["norm"])
        r = R.guard_ref(h, max_norm=1.0, skip_nonfinite=False)
        assert r["skip"] == 0 and not math.isfinite(r["norm"])
    half = R.guard_ref(g, 1.0, R.guard_ref(g)["norm"] / 2)
    assert abs(half["coef"] - 0.5) < 1e-6
    tiny = np.full(8, 1e-40, np.float32)                                  # subnormal gradients count
    assert abs(R.guard_ref(tiny)["norm"] / (math.sqrt(8) * float(np.float32(1e-40))) - 1) < 1e-12
    assert abs(R.kernel_norm(tiny, 1.0) - R.guard_ref(tiny)["norm"]) <= 2.0 ** -150
