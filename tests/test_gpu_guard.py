"""The step guard on a real MI355X: ``avid_grad_guard`` against float64 (tests/_guard_ref.py) inside the bound DESIGN.md 3.8d
derives, its verdict on non-finite gradients, the guarded optimizers (bit for bit the unguarded ones when nothing is
clipped, nothing written on a skip), ``avid_guard_restore``, and the three step engines with the options on: a skipped step
leaves no trace, eagerly, over virtual ranks and in a captured graph."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import _guard_ref as R

pytestmark = pytest.mark.gpu

PATTERN = -7.25                     # what guard bands and must-not-be-written buffers are filled with
U32 = 2.0 ** -24


def _bits(t):
    t = torch.from_numpy(t) if isinstance(t, np.ndarray) else t.detach().cpu()
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rand(n, seed, scale=1.0):
    return scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _seated(values, start, dev, fill=float("nan")):
    """``values`` on the device, ``start`` floats behind a 16-byte boundary, inside a buffer otherwise full of ``fill`` (NaN:
    a read outside the slice poisons the sum).  Returns (slice, whole buffer)."""
    n = values.numel()
    whole = torch.full((n + 12,), fill, dtype=torch.float32, device=dev)
    assert whole.data_ptr() % 16 == 0
    s = whole[4 + start:4 + start + n]
    s.copy_(values)
    return s, whole


def _read(guard):
    torch.cuda.synchronize()
    r = guard.record.cpu()
    return {"norm": float(r.view(torch.float32)[0]), "coef": float(r.view(torch.float32)[1]), "skip": int(r[2]),
            "reserved": int(r[3]), "skipped_total": int(r.view(torch.int64)[2]), "steps_total": int(r.view(torch.int64)[3]),
            "bits": r[:3].clone()}


def _set(guard, coef, skip):
    guard.record.zero_()
    guard.record.view(torch.float32)[1] = coef
    guard.record[2] = skip


# ------------------------------------------------------------------------------------------------------------------ avid_grad_guard
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1023, 4097, R.GRID_STRIDE + 1029])
def test_grad_guard_against_float64(gpu_device, n):
    """Slices 0 .. 3 floats behind a 16-byte boundary (scalar head and tail of every length), surrounded by NaN; n up to one
    element-round past a full grid stride.  grad_norm within the derived bound, clip_coef within it plus one rounding, 1.0
    exactly when the norm is under max_norm; the same bits twice."""
    from avid_hip import ops
    dev = gpu_device
    guard = ops.StepGuard(dev)
    scale = 0.5
    bound = R.norm_bound(n)
    for start in range(4):
        g = _rand(n, 40 + start)
        gd, whole = _seated(g, start, dev)
        ref = R.guard_ref(g.numpy(), scale)
        max_norm = float(np.float32(0.25 * ref["norm"]))
        ref = R.guard_ref(g.numpy(), scale, max_norm)
        ops.grad_guard(gd, guard, scale, max_norm, True)
        got = _read(guard)
        err_n = abs(got["norm"] - ref["norm"]) / ref["norm"]
        err_c = abs(got["coef"] - ref["coef"]) / ref["coef"]
        print(f"\n[grad_guard] n {n} start {start}: norm {got['norm']!r} (float64 {ref['norm']!r}) rel {err_n:.3e} bound {bound:.3e}; "
              f"coef {got['coef']!r} (float64 {ref['coef']!r}) rel {err_c:.3e}")
        assert err_n <= bound, (n, start, err_n)
        assert err_c <= (1 + bound) * (1 + U32) - 1 + 2.0 ** -50, (n, start, err_c)
        assert got["skip"] == 0 and got["reserved"] == 0 and 0.2 < got["coef"] < 0.3
        assert got["norm"] == R.kernel_norm(g.numpy(), scale, start), "the kernel is not the summation the bound was derived for"
        ops.grad_guard(gd, guard, scale, max_norm, True)                      # the same bits run to run
        again = _read(guard)
        assert torch.equal(again["bits"], got["bits"]) and again["steps_total"] == got["steps_total"] + 1
        ops.grad_guard(gd, guard, scale, 2 * ref["norm"], True)               # under max_norm: exactly 1.0
        loose = _read(guard)
        assert loose["coef"] == 1.0 and loose["norm"] == got["norm"]
        ops.grad_guard(gd, guard, scale, 0.0, False)                          # no clipping asked for
        assert _read(guard)["coef"] == 1.0
        assert bool(torch.isnan(whole[:4 + start]).all()) and bool(torch.isnan(whole[4 + start + n:]).all())
    assert _read(guard)["steps_total"] == 16 and _read(guard)["skipped_total"] == 0


def test_grad_guard_zero_and_subnormal_gradients(gpu_device):
    from avid_hip import ops
    dev = gpu_device
    guard = ops.StepGuard(dev)
    for n, start in ((1, 0), (4097, 1)):
        z, _ = _seated(torch.zeros(n), start, dev)
        ops.grad_guard(z, guard, 1.0, 1.0, True)
        got = _read(guard)
        assert got["norm"] == 0.0 and got["coef"] == 1.0 and got["skip"] == 0
        # subnormal gradients (their squares are far below fp32, and below nothing in double): summed, not flushed
        tiny = torch.full((n,), 1e-40) * (1 + torch.arange(n) % 3)
        assert float(tiny.abs().max()) < 2.0 ** -126
        t, _ = _seated(tiny, start, dev)
        ops.grad_guard(t, guard, 1.0, 0.0, True)
        got, ref = _read(guard), R.guard_ref(tiny.numpy())
        assert ref["norm"] > 0 and abs(got["norm"] - ref["norm"]) <= R.norm_bound(n) * ref["norm"] + 2.0 ** -150, (got, ref)
        assert got["skip"] == 0


@pytest.mark.parametrize("start", [0, 1])
def test_grad_guard_judges_non_finite_gradients(gpu_device, start):
    """n = 4097: at start 0 no head and a tail of one, at start 1 a head of three and a tail of two.  nan, +inf, -inf and 3e19
    (finite; its square overflows fp32) at the first, the last, a head, a tail and a middle element."""
    from avid_hip import ops
    dev, n = gpu_device, 4097
    head, n4, tail = R.partition(n, start)
    assert (head, tail) == ((0, 1) if start == 0 else (3, 2))
    spots = sorted({0, n - 1, max(head - 2, 0), n - tail, n // 2})
    g = _rand(n, 5)
    guard, loose = ops.StepGuard(dev), ops.StepGuard(dev)
    count = 0
    for spot in spots:
        for poison in (float("nan"), float("inf"), -float("inf"), 3e19):
            h = g.clone()
            h[spot] = poison
            hd, _ = _seated(h, start, dev)
            ops.grad_guard(hd, guard, 1.0, 1.0, True)
            got = _read(guard)
            count += 1
            assert (got["skip"], got["coef"], got["skipped_total"], got["steps_total"]) == (1, 1.0, count, count), (spot, poison, got)
            assert not math.isfinite(got["norm"]) and math.isnan(got["norm"]) == math.isnan(poison)
            ops.grad_guard(hd, loose, 1.0, 0.0, False)
            got = _read(loose)
            assert got["skip"] == 0 and got["skipped_total"] == 0 and not math.isfinite(got["norm"]), (spot, poison, got)
    hd, _ = _seated(g, start, dev)
    ops.grad_guard(hd, guard, 1.0, 1.0, True)                                  # a clean one behind them
    got = _read(guard)
    assert got["skip"] == 0 and got["skipped_total"] == count and got["steps_total"] == count + 1 and got["coef"] < 1.0


# ------------------------------------------------------------------------------------------------------------------ guarded optimizers
HYPER = (2e-4, 0.9, 0.999, 1e-8, 1e-5)          # lr, betas, eps, weight decay
SGD_FORMS = ((0.0, False), (0.9, False), (0.9, True))


def _banded(values, off, dev):
    """``values`` at element ``off`` (a multiple of 4: the optimizers take 16-byte aligned buffers) of a PATTERN-filled buffer."""
    s, whole = _seated(values, 0, dev, PATTERN)
    if off:
        whole = torch.full((values.numel() + 12 + off,), PATTERN, dtype=torch.float32, device=dev)
        s = whole[4 + off:4 + off + values.numel()]
        s.copy_(values)
    return s, whole


def _bands_intact(whole, s):
    lo = (s.data_ptr() - whole.data_ptr()) // 4
    return bool((whole[:lo] == PATTERN).all()) and bool((whole[lo + s.numel():] == PATTERN).all())


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_guarded_optimizers_unclipped_are_the_unguarded_kernels(gpu_device, n, off):
    """skip == 0 and clip_coef == 1.0f: two steps of Adam (grad_scale 1/3, by-value and device step) and of the three SGD
    forms, bit for bit ``avid_adam_flat`` / ``avid_sgd_flat``; at the start of an allocation and 16 bytes into one."""
    from avid_hip import ops
    dev = gpu_device
    guard = ops.StepGuard(dev)
    _set(guard, 1.0, 0)
    p0, grads = _rand(n, 1), [_rand(n, 10 + s, 0.3).to(dev) for s in range(2)]
    for use_dev in (False, True):
        (p, wp), (m, wm), (v, wv) = (_banded(t, off, dev) for t in (p0, torch.zeros(n), torch.zeros(n)))
        p2, m2, v2 = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        t1 = torch.zeros((), dtype=torch.int64, device=dev) if use_dev else None
        t2 = torch.zeros((), dtype=torch.int64, device=dev) if use_dev else None
        for s, g in enumerate(grads):
            gs, _ = _banded(g, off, dev)
            ops.adam_flat_guarded(p, gs, m, v, *HYPER, 0 if use_dev else s + 1, guard, grad_scale=1 / 3, step_dev=t1)
            ops.adam_flat(p2, g, m2, v2, *HYPER, 0 if use_dev else s + 1, grad_scale=1 / 3, step_dev=t2)
            assert _same_bits(p, p2) and _same_bits(m, m2) and _same_bits(v, v2), (use_dev, s)
        assert all(_bands_intact(w, s) for w, s in ((wp, p), (wm, m), (wv, v)))
        assert not use_dev or int(t1) == int(t2) == 2
    for momentum, nesterov in SGD_FORMS:
        (p, wp), (b, wb) = _banded(p0, off, dev), _banded(torch.zeros(n), off, dev)
        p2, b2 = p0.to(dev), torch.zeros(n, device=dev)
        for s, g in enumerate(grads):
            gs, _ = _banded(g, off, dev)
            ops.sgd_flat_guarded(p, gs, b if momentum else None, 0.1, momentum, 1e-4, guard, nesterov, grad_scale=1 / 3)
            ops.sgd_flat(p2, g, b2 if momentum else None, 0.1, momentum, 1e-4, nesterov, grad_scale=1 / 3)
            assert _same_bits(p, p2) and _same_bits(b, b2), (momentum, nesterov, s)
        assert _bands_intact(wp, p) and _bands_intact(wb, b)


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_guarded_optimizers_apply_the_coefficient(gpu_device, n, off):
    """clip_coef = 0.37 written into the record.  SGD: bit for bit torch's fp32 single-tensor arithmetic (tests/_sgd_ref.py) on
    (g * scale) * coef, the products rounded one after the other.  Adam: float64 within tests/test_gpu_ops.py::test_adam_flat's
    tolerance."""
    from avid_hip import ops
    dev = gpu_device
    guard = ops.StepGuard(dev)
    _set(guard, 0.37, 0)
    coef = float(np.float32(0.37))
    scale = 1 / 3
    p0, grads = _rand(n, 2), [_rand(n, 20 + s, 0.3) for s in range(3)]
    for momentum, nesterov in SGD_FORMS:
        for wd in (0.0, 1e-4):
            (p, wp), (b, wb) = _banded(p0, off, dev), _banded(torch.zeros(n), off, dev)
            rp, rb = p0.numpy(), (np.zeros(n, np.float32) if momentum else None)
            for s, g in enumerate(grads):
                gs, _ = _banded(g, off, dev)
                ops.sgd_flat_guarded(p, gs, b if momentum else None, 0.1, momentum, wd, guard, nesterov, grad_scale=scale)
                rp, rb = R.sgd_clipped(rp, g.numpy(), rb, 0.1, momentum, wd, nesterov, scale, coef)
                assert _same_bits(p, rp) and (rb is None or _same_bits(b, rb)), (momentum, nesterov, wd, s)
            assert _bands_intact(wp, p) and _bands_intact(wb, b)
            if not momentum:
                assert bool((b == 0).all())                                # no momentum: its buffer is not touched
    (p, wp), (m, wm), (v, wv) = (_banded(t, off, dev) for t in (p0, torch.zeros(n), torch.zeros(n)))
    rp, rm, rv = p0.double().numpy(), np.zeros(n), np.zeros(n)
    t_dev = torch.zeros((), dtype=torch.int64, device=dev)
    for s, g in enumerate(grads):
        gs, _ = _banded(g, off, dev)
        ops.adam_flat_guarded(p, gs, m, v, *HYPER, 0, guard, grad_scale=scale, step_dev=t_dev)
        rp, rm, rv = R.adam_clipped(rp, g.numpy(), rm, rv, *HYPER, s + 1, scale, coef)
    np.testing.assert_allclose(p.cpu().numpy(), rp, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(m.cpu().numpy(), rm, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(v.cpu().numpy(), rv, rtol=1e-6, atol=1e-7)
    assert int(t_dev) == 3 and all(_bands_intact(w, s) for w, s in ((wp, p), (wm, m), (wv, v)))
    # ... and the coefficient is really in there: an unclipped step from the same start lands elsewhere
    q, qm, qv = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for s, g in enumerate(grads):
        ops.adam_flat(q, g.to(dev), qm, qv, *HYPER, s + 1, grad_scale=scale)
    assert not _same_bits(qm, m)


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_guarded_optimizers_write_nothing_on_a_skip(gpu_device, n, off):
    """skip == 1 (and a NaN gradient, a coefficient that would show): p, m, v, buf and the step counter keep their bits,
    PATTERN-filled buffers keep the pattern."""
    from avid_hip import ops, lib
    dev = gpu_device
    guard = ops.StepGuard(dev)
    _set(guard, 0.37, 1)
    p0, m0, v0 = _rand(n, 3), _rand(n, 4, 0.1), _rand(n, 5, 0.1).abs()
    g, _ = _banded(torch.full((n,), float("nan")), off, dev)
    (p, wp), (m, wm), (v, wv) = (_banded(t, off, dev) for t in (p0, m0, v0))
    t_dev = torch.full((), 41, dtype=torch.int64, device=dev)
    ops.adam_flat_guarded(p, g, m, v, *HYPER, 0, guard, step_dev=t_dev)
    assert _same_bits(p, p0) and _same_bits(m, m0) and _same_bits(v, v0) and int(t_dev) == 41
    for momentum, nesterov in SGD_FORMS:
        ops.sgd_flat_guarded(p, g, m if momentum else None, 0.1, momentum, 1e-4, guard, nesterov)
        assert _same_bits(p, p0) and _same_bits(m, m0)
    full = [torch.full((n,), PATTERN, device=dev) for _ in range(3)]
    ops.adam_flat_guarded(full[0], g, full[1], full[2], *HYPER, 7, guard)
    ops.sgd_flat_guarded(full[0], g, full[1], 0.1, 0.9, 1e-4, guard, True)
    assert all(bool((t == PATTERN).all()) for t in full)
    assert all(_bands_intact(w, s) for w, s in ((wp, p), (wm, m), (wv, v)))
    _set(guard, 1.0, 0)                                                       # the counter's guarded form, both ways
    lib.call("avid_counter_add_unless", ops._p(t_dev), 3, ops._p(guard.record), ops._stream())
    assert int(t_dev) == 44
    _set(guard, 1.0, 1)
    lib.call("avid_counter_add_unless", ops._p(t_dev), 3, ops._p(guard.record), ops._stream())
    assert int(t_dev) == 44


def test_guarded_optimizers_take_what_the_unguarded_ones_take(gpu_device):
    """16-byte aligned buffers, as ``avid_adam_flat`` / ``avid_sgd_flat``: a slice one float in is refused, nothing is written."""
    from avid_hip import ops, AvidHipError
    dev = gpu_device
    guard = ops.StepGuard(dev)
    _set(guard, 1.0, 0)
    x = [torch.full((16,), PATTERN, device=dev) for _ in range(4)]
    with pytest.raises(AvidHipError, match="16-byte"):
        ops.adam_flat_guarded(x[0][1:9], x[1][1:9], x[2][1:9], x[3][1:9], *HYPER, 1, guard)
    with pytest.raises(AvidHipError, match="16-byte"):
        ops.sgd_flat_guarded(x[0][1:9], x[1][1:9], x[2][1:9], 0.1, 0.9, 0.0, guard)
    torch.cuda.synchronize()
    assert all(bool((t == PATTERN).all()) for t in x)


# ------------------------------------------------------------------------------------------------------------------ avid_guard_restore
@pytest.mark.parametrize("D", [128, 100])
def test_guard_restore(gpu_device, D):
    from avid_hip import ops
    dev, N = gpu_device, 50
    guard = ops.StepGuard(dev)
    before = _rand(N * D, 6).view(N, D).to(dev)
    idx = torch.tensor([3, 7, 3, 49, 0, 7, 3], device=dev)                   # duplicates: saved with the same pre-update row
    saved = before.index_select(0, idx)
    after = before.clone()
    after[idx.unique()] = PATTERN
    untouched = torch.ones(N, dtype=torch.bool, device=dev)
    untouched[idx] = False
    for skip in (0, 1):
        _set(guard, 1.0, skip)
        dst = after.clone()
        ops.guard_restore(dst, idx, saved, guard)
        assert _same_bits(dst, before if skip else after)
        assert _same_bits(dst[untouched], before[untouched])
        flat = torch.full((N * D,), PATTERN, device=dev)                     # idx None: a flat copy
        ops.guard_restore(flat, None, before.view(-1), guard)
        assert _same_bits(flat, before.view(-1)) if skip else bool((flat == PATTERN).all())
        odd = torch.full((N * D + 8,), PATTERN, device=dev)                  # ... of a 4-byte aligned slice, bands intact
        ops.guard_restore(odd[3:3 + 77], None, before.view(-1)[5:5 + 77], guard)
        assert bool((odd[:3] == PATTERN).all()) and bool((odd[80:] == PATTERN).all())
        assert _same_bits(odd[3:80], before.view(-1)[5:82]) if skip else bool((odd == PATTERN).all())


def test_guard_nonfinite_is_a_second_witness(gpu_device):
    """A non-finite element anywhere in a small buffer turns a clean record into a skip (once: a record that already says skip
    keeps its count); a finite buffer changes nothing; nothing outside the slice is read."""
    from avid_hip import ops
    dev, n = gpu_device, 19507
    guard = ops.StepGuard(dev)
    clean = _rand(n, 8)
    for start in (0, 1):
        x, _ = _seated(clean, start, dev)
        _set(guard, 0.37, 0)
        ops.guard_nonfinite(x, guard)
        got = _read(guard)
        assert (got["skip"], got["skipped_total"]) == (0, 0) and abs(got["coef"] - 0.37) < 1e-7
        for spot in (0, 255, 256, n // 2, n - 1):
            for poison in (float("nan"), float("inf"), -float("inf")):
                h = clean.clone()
                h[spot] = poison
                x, _ = _seated(h, start, dev)
                _set(guard, 0.37, 0)
                ops.guard_nonfinite(x, guard)
                got = _read(guard)
                assert (got["skip"], got["coef"], got["skipped_total"], got["steps_total"]) == (1, 1.0, 1, 0), (spot, poison, got)
                ops.guard_nonfinite(x, guard)                                  # already a skip: counted once
                assert _read(guard)["skipped_total"] == 1


# ------------------------------------------------------------------------------------------------------------------ TrainStep
def _engine(dev, **opts):
    """tests/test_gpu_engine.py's model, banks (N = 5000, K = 256) and sampler seed under a TrainStep with ``opts``."""
    import test_gpu_engine as E
    from avid_hip.parallel import TrainStep
    m, crit, _ = E._make(dev)
    return m, crit, TrainStep(m, crit, **opts)


def _batch(dev, steps=6):
    import test_gpu_engine as E
    return E._data(dev, steps=steps)


def _poisoned(video, sample=1):
    bad = video.clone()
    bad[sample, 1, 3, 17, 29] = float("inf")
    return bad


def _state(m, crit, eng):
    """Everything a skipped step must leave alone, cloned."""
    st = {"params": eng.flat.flat.clone(), "stats": eng.flat_buffers.flat.clone(),
          "nbt": torch.stack([mod.num_batches_tracked for mod in m.modules() if getattr(mod, "num_batches_tracked", None) is not None]),
          "bank1": crit.nce_average.view1_mem.clone(), "bank2": crit.nce_average.view2_mem.clone()}
    if eng.m is not None:
        st.update(m=eng.m.clone(), v=eng.v.clone(), t_dev=eng.t_dev.clone())
    return st


def _assert_same_state(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]) and _same_bits(a[k], b[k]) if a[k].is_floating_point() else torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def plain_run(gpu_device):
    """Three steps of the engine as it always was: the losses and the state behind each step."""
    video, audio, ids = _batch(gpu_device)
    m, crit, eng = _engine(gpu_device)
    assert eng.guard is None
    losses, states = [], []
    for i in range(3):
        losses.append(float(eng.step(video, audio, ids[i])))
        states.append(_state(m, crit, eng))
    return losses, states


def test_trainstep_guard_that_never_fires_changes_nothing(gpu_device, plain_run):
    """(a) max_grad_norm = 1e30, skip_nonfinite: three steps with the losses, parameters, moments, statistics and banks of the
    plain engine, bit for bit (one optimizer launch where the plain step runs two slices: the same arithmetic per element)."""
    video, audio, ids = _batch(gpu_device)
    m, crit, eng = _engine(gpu_device, max_grad_norm=1e30, skip_nonfinite=True)
    losses, states = plain_run
    for i in range(3):
        assert float(eng.step(video, audio, ids[i])) == losses[i]
        _assert_same_state(_state(m, crit, eng), states[i])
    assert eng._step_plan is not None, "the step did not run through a launch program"
    g = eng.guard
    assert int(g.skipped) == 0 and int(g.skipped_total) == 0 and int(g.steps_total) == 3 and float(g.clip_coef) == 1.0
    assert 0 < float(g.grad_norm) < 1e30
    assert eng.t == 3 and int(eng.t_dev) == 3 and not crit.nce_average.keep_rows and crit.nce_average.kept_rows is None


def test_trainstep_skips_a_poisoned_step_without_a_trace(gpu_device, plain_run):
    """(b) step 3 sees one inf in its video: skipped; parameters, moments, t_dev, running statistics, every
    num_batches_tracked and both banks are what step 2 left.  A fourth, clean step trains."""
    video, audio, ids = _batch(gpu_device)
    m, crit, eng = _engine(gpu_device, skip_nonfinite=True)
    for i in range(2):
        eng.step(video, audio, ids[i])
    before = _state(m, crit, eng)
    _assert_same_state(before, plain_run[1][1])
    eng.step(_poisoned(video), audio, ids[2])       # (its loss may well be finite: a ReLU turns the NaN channel into zeros)
    g = eng.guard
    assert int(g.skipped) == 1 and int(g.skipped_total) == 1 and int(g.steps_total) == 3 and not math.isfinite(float(g.grad_norm))
    _assert_same_state(_state(m, crit, eng), before)
    assert eng.t == 3 and int(eng.t_dev) == 2 and eng.state_dict()["state"][0]["step"] == 2.0
    assert crit.nce_average.multinomial.offset == 3                          # the sampler's position went on
    loss = eng.step(video, audio, ids[3])
    assert math.isfinite(float(loss)) and int(g.skipped) == 0 and int(g.skipped_total) == 1
    after = _state(m, crit, eng)
    assert not torch.equal(after["params"], before["params"]) and int(eng.t_dev) == 3
    assert bool(torch.isfinite(after["params"]).all()) and bool(torch.isfinite(after["bank1"]).all())
    assert bool(torch.isfinite(after["stats"]).all()) and torch.equal(after["nbt"], before["nbt"] + 1)
    assert not torch.equal(after["bank1"][ids[3]], before["bank1"][ids[3]])


def test_trainstep_poisoned_first_step_leaves_z_unfrozen(gpu_device, plain_run):
    """(c) the step that would freeze Z is skipped: Z is estimated again by the next, clean one."""
    video, audio, ids = _batch(gpu_device)
    m, crit, eng = _engine(gpu_device, skip_nonfinite=True)
    before = _state(m, crit, eng)
    eng.step(_poisoned(video), audio, ids[0])
    assert int(eng.guard.skipped) == 1
    _assert_same_state(_state(m, crit, eng), before)
    assert not crit.criterion.z_ready() and float(crit.criterion.avg_exp_score) == -1.0
    loss = eng.step(video, audio, ids[0])
    z = float(crit.criterion.avg_exp_score)
    assert crit.criterion.z_ready() and math.isfinite(z) and z > 0 and math.isfinite(float(loss))
    assert int(eng.guard.skipped) == 0 and int(eng.t_dev) == 1 and eng.t == 2
    # the first step of the plain engine from the same state, but for the sampler's position (it went on)
    assert torch.equal(_state(m, crit, eng)["stats"], plain_run[1][0]["stats"])


def test_trainstep_clips_to_half_the_norm(gpu_device):
    """(d) max_grad_norm = half the norm a first run reported: clip_coef is the float64 coefficient of the engine's own
    gradient (within the norm's bound plus one rounding, about 0.5), and forward_backward() + optimizer_step() is float64
    Adam on that gradient times that coefficient, within test_adam_flat's tolerance."""
    video, audio, ids = _batch(gpu_device)
    m, crit, eng = _engine(gpu_device, max_grad_norm=1e30)
    eng.forward_backward(video, audio, ids[0])
    norm0 = float(eng.guard.grad_norm)
    assert math.isfinite(norm0) and norm0 > 0 and float(eng.guard.clip_coef) == 1.0
    m, crit, eng = _engine(gpu_device, max_grad_norm=norm0 / 2)
    eng.forward_backward(video, audio, ids[0])
    grad, p0 = eng.flat.grad.cpu().numpy(), eng.flat.flat.cpu().double().numpy()
    ref = R.guard_ref(grad, 1.0, norm0 / 2)
    got_norm, got_coef = float(eng.guard.grad_norm), float(eng.guard.clip_coef)
    bound = R.norm_bound(grad.size)
    print(f"\n[trainstep clip] n {grad.size}: norm {got_norm!r} (float64 {ref['norm']!r}), coef {got_coef!r} (float64 {ref['coef']!r})")
    assert got_norm == norm0 and abs(got_norm - ref["norm"]) <= bound * ref["norm"]
    assert abs(got_coef - ref["coef"]) <= ((1 + bound) * (1 + U32) - 1 + 2.0 ** -50) * ref["coef"] and abs(got_coef - 0.5) < 2e-3
    eng.optimizer_step()
    want, wm, wv = R.adam_clipped(p0, grad, np.zeros_like(p0), np.zeros_like(p0), eng.lr, *eng.betas, eng.eps, eng.wd, 1, 1.0,
                                  ref["coef"])
    np.testing.assert_allclose(eng.flat.flat.cpu().numpy(), want, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(eng.m.cpu().numpy(), wm, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(eng.v.cpu().numpy(), wv, rtol=1e-6, atol=1e-12)
    assert int(eng.t_dev) == 1 and int(eng.guard.skipped) == 0


def test_trainstep_virtual_ranks_skip(gpu_device):
    """(e) virtual_ranks = 2 at global batch 4, the inf in shard 1: the whole step is skipped — the banks (one deferred
    update of all four records) and rank 0's running statistics are put back, like everything else."""
    video, audio, ids = _batch(gpu_device)
    m, crit, eng = _engine(gpu_device, virtual_ranks=2, skip_nonfinite=True)
    eng.step(video, audio, ids[0])
    assert int(eng.guard.skipped) == 0
    before = _state(m, crit, eng)
    eng.step(_poisoned(video, sample=3), audio, ids[1])
    assert int(eng.guard.skipped) == 1 and math.isfinite(float(eng.rank_losses[0]))
    _assert_same_state(_state(m, crit, eng), before)
    loss = eng.step(video, audio, ids[2])
    after = _state(m, crit, eng)
    assert math.isfinite(float(loss)) and int(eng.t_dev) == 2 and not torch.equal(after["params"], before["params"])
    assert torch.equal(after["nbt"], before["nbt"] + 1) and not torch.equal(after["bank2"][ids[2]], before["bank2"][ids[2]])


def test_trainstep_captured_graph_obeys_the_guard(gpu_device):
    """(f) captured after two eager steps; replays of a clean, a poisoned and a clean batch: the poisoned replay changes
    nothing, skipped_total == 1, t_dev ends two above its value at capture.  Nothing in the graph waits for the host."""
    video, audio, ids = _batch(gpu_device)
    m, crit, eng = _engine(gpu_device, max_grad_norm=1e30, skip_nonfinite=True)
    for i in range(2):
        eng.step(video, audio, ids[i])
    eng.capture(video, audio, ids[2])
    t0 = int(eng.t_dev)
    assert t0 == 2 and int(eng.guard.steps_total) == 2
    loss = eng.replay(video, audio, ids[2])
    assert math.isfinite(float(loss)) and int(eng.t_dev) == 3
    before = _state(m, crit, eng)
    eng.replay(_poisoned(video), audio, ids[3])
    assert int(eng.guard.skipped) == 1 and not math.isfinite(float(eng.guard.grad_norm))
    _assert_same_state(_state(m, crit, eng), before)
    loss = eng.replay(video, audio, ids[4])
    assert math.isfinite(float(loss)) and int(eng.guard.skipped) == 0
    assert int(eng.guard.skipped_total) == 1 and int(eng.guard.steps_total) == 5 and int(eng.t_dev) == t0 + 2 and eng.t == 5
    after = _state(m, crit, eng)
    assert not torch.equal(after["params"], before["params"]) and bool(torch.isfinite(after["params"]).all())
    assert bool(torch.isfinite(after["bank1"]).all()) and bool(torch.isfinite(after["stats"]).all())


# ------------------------------------------------------------------------------------------------------------------ the supervised engines
def _supervised(eng, m, vids, labs, state):
    """clean, poisoned, clean: the poisoned step leaves ``state()`` alone, the clean ones train."""
    eng.step(vids[0], labs[0])
    assert int(eng.guard.skipped) == 0 and 0 < float(eng.guard.clip_coef) <= 1.0
    before = state()
    bad = vids[1].clone()
    bad[0, 2, 1, 5, 7] = float("inf")
    eng.step(bad, labs[1])
    assert int(eng.guard.skipped) == 1 and int(eng.guard.skipped_total) == 1 and float(eng.guard.clip_coef) == 1.0
    for a, b in zip(state(), before):
        assert torch.equal(a, b)
    loss = eng.step(vids[2], labs[2])[0]
    assert int(eng.guard.skipped) == 0 and bool(torch.isfinite(loss).all())
    after = state()
    assert all(bool(torch.isfinite(t).all()) for t in after if t.is_floating_point())
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1]) and not torch.equal(after[2], before[2])
    assert torch.equal(after[3], before[3] + 1)


def _nbt(m):
    return torch.stack([mod.num_batches_tracked for mod in m.modules() if getattr(mod, "num_batches_tracked", None) is not None])


def test_finetunestep_sgd_skips_and_clips(gpu_device):
    import test_gpu_finetune as FT
    from avid_hip import parallel
    dev = gpu_device
    g = torch.Generator().manual_seed(3)
    vids = [torch.randn((4, 3, 8, 112, 112), generator=g).to(dev) for _ in range(3)]
    labs = [torch.randint(0, 101, (4,), generator=g).to(dev) for _ in range(3)]
    m = FT._wrapper(dev)
    eng = parallel.FinetuneStep(m, lr=1e-3, optimizer="sgd", momentum=0.9, max_grad_norm=1.0, skip_nonfinite=True)
    _supervised(eng, m, vids, labs, lambda: [eng.flat.flat.clone(), eng.momentum_buffer.clone(), eng.flat_buffers.flat.clone(),
                                             _nbt(m), m.classifier.weight.detach().clone()])


def test_probestep_skips_and_clips(gpu_device):
    """The tower is frozen and its ReLUs turn a NaN channel into zeros: the heads' gradient stays finite.  What gives the step
    away is the tower's running statistics (``avid_guard_nonfinite``)."""
    import test_gpu_probe as PR
    from avid_hip import parallel
    dev = gpu_device
    g = torch.Generator().manual_seed(9)
    vids = [torch.randn((2, 3, 8, 64, 64), generator=g).to(dev) for _ in range(3)]
    labs = [torch.randint(0, 400, (2,), generator=g).to(dev) for _ in range(3)]
    m = PR._model(dev)
    eng = parallel.ProbeStep(m, lr=1e-3, optimizer="sgd", momentum=0.9, max_grad_norm=1.0, skip_nonfinite=True)
    _supervised(eng, m, vids, labs, lambda: [eng.flat.flat.clone(), eng.momentum_buffer.clone(), eng.flat_buffers.flat.clone(),
                                             _nbt(m)])


# ------------------------------------------------------------------------------------------------------------------ resources
def test_new_kernels_keep_everything_in_registers():
    """No spilled register and no private segment in any of the guard's kernels (read from the code objects: no GPU work)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from kernel_resources import kernel_table
    names = ("grad_sumsq_kernel", "grad_guard_finish_kernel", "counter_add_unless_kernel", "guard_restore_kernel",
             "guard_nonfinite_kernel",
             "adam_flat_kernel", "adam_flat_guarded_kernel", "adam_flat_ema_kernel", "adam_flat_ema_guarded_kernel",
             "sgd_flat_kernel", "sgd_flat_guarded_kernel", "sgd_flat_ema_kernel", "sgd_flat_ema_guarded_kernel")
    rows = {r["name"]: r for r in kernel_table() if r["name"] in names}
    assert sorted(rows) == sorted(names)
    for name, r in rows.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert not r["uses_dynamic_stack"], name
