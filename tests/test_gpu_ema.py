"""The weight average on a real MI355X: the averaging forms of the optimizer kernels against the plain kernels (p, m, v, buf: the
same bits) and the numpy restatement (tests/_ema_ref.py: e, bit for bit), ``avid_ema_flat`` and ``avid_swap_flat``, guard bands,
the step engines against an independent recomputation from per-step snapshots, the step guard, a captured graph,
``ema_weights()`` and checkpoints."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from _ema_ref import ema_sequence, ema_update

pytestmark = pytest.mark.gpu

BIG = 4 * 256 * 4096 + 7      # the grid-stride loop's second round (4096 blocks x 256 threads x 4 floats) and a tail
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-5)
SGDS = ((0.0, False, 0.0), (0.9, True, 0.0), (0.9, False, 1e-4))          # (momentum, nesterov, weight decay)
GUARDS = (None, (1.0, 0), (0.37, 0), (1.0, 1))                            # unguarded, (clip_coef, skip)
AVERAGES = ((0.0, False, None), (0.9, False, None), (0.9999, False, None), (0.999, True, 0), (0.999, True, 5), (0.999, True, 10 ** 6))


def _bits(t):
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t.detach().cpu()
    return t.contiguous().view(torch.int32)


def _same_bits(got, want):
    if isinstance(got, torch.Tensor) and isinstance(want, torch.Tensor) and got.device == want.device:
        return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    return torch.equal(_bits(got), _bits(want))


def _same(a, b):
    """Floating-point tensors bit for bit, anything else by value."""
    return _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)


def _rand(n, seed, scale=1.0):
    return scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _guard(dev, spec):
    from avid_hip import ops
    if spec is None:
        return None
    g = ops.StepGuard(dev)
    g.record.view(torch.float32)[1] = spec[0]
    g.record[2] = spec[1]
    return g


def _cases(n):
    """Every guard form x every averaging form; at the large size one decay and one warm-up count per guard form."""
    avgs = AVERAGES if n < BIG else (AVERAGES[1], AVERAGES[4])
    return [(g, a) for g in GUARDS for a in avgs]


def _counter(dev, k):
    return None if k is None else torch.full((), k, dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, BIG])
def test_adam_with_the_average_is_adam_and_the_restatement(gpu_device, n):
    """Two successive steps (the second with moments that are not zero), by-value step count and the device counter: p, m, v
    are the bits of adam_flat / adam_flat_guarded on the same inputs, e is the restatement applied to those p; a skip leaves
    everything — the counter included — alone."""
    from avid_hip import ops
    dev = gpu_device
    p0, e0 = _rand(n, 1), _rand(n, 2)
    grads = [_rand(n, 10 + s, 0.3).to(dev) for s in range(2)]
    bad = []
    for spec, (decay, warmup, k0) in _cases(n):
        for use_dev in ((False, True) if n < BIG else (True,)):
            guard = _guard(dev, spec)
            pa, ma, va = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            pb, mb, vb, e = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), e0.to(dev)
            ta = torch.zeros((), dtype=torch.int64, device=dev) if use_dev else None
            tb = torch.zeros((), dtype=torch.int64, device=dev) if use_dev else None
            upd = _counter(dev, k0)
            want_e, k = e0.numpy(), (k0 or 0)
            for s in range(2):
                args = (ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], ADAM["wd"], s + 1)
                if guard is None:
                    ops.adam_flat(pa, grads[s], ma, va, *args, grad_scale=0.5, step_dev=ta)
                else:
                    ops.adam_flat_guarded(pa, grads[s], ma, va, *args, guard, grad_scale=0.5, step_dev=ta)
                ops.adam_flat_ema(pb, grads[s], mb, vb, e, *args, decay, guard=guard, grad_scale=0.5, step_dev=tb, warmup=warmup,
                                  updates_dev=upd)
                skipped = spec is not None and spec[1]
                if not skipped:
                    want_e = ema_update(want_e, pa.cpu().numpy(), decay, k, warmup)
                    k += 1
                ok = (_same_bits(pb, pa) and _same_bits(mb, ma) and _same_bits(vb, va) and _same_bits(e, want_e)
                      and (upd is None or int(upd) == k) and (tb is None or int(tb) == int(ta)))
                if skipped:
                    ok = ok and _same_bits(pb, p0) and not bool(mb.any()) and not bool(vb.any()) and _same_bits(e, e0) and (tb is None or int(tb) == 0)
                if not ok:
                    bad.append((spec, decay, warmup, k0, use_dev, s))
                    break
    assert not bad, bad


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, BIG])
def test_sgd_with_the_average_is_sgd_and_the_restatement(gpu_device, n):
    from avid_hip import ops
    dev = gpu_device
    p0, e0 = _rand(n, 3), _rand(n, 4)
    grads = [_rand(n, 20 + s, 0.3).to(dev) for s in range(2)]
    bad = []
    for momentum, nesterov, wd in (SGDS if n < BIG else SGDS[1:2]):
        for spec, (decay, warmup, k0) in _cases(n):
            guard = _guard(dev, spec)
            pa, pb, e = p0.to(dev), p0.to(dev), e0.to(dev)
            ba = torch.zeros(n, device=dev) if momentum else None
            bb = torch.zeros(n, device=dev) if momentum else None
            upd = _counter(dev, k0)
            want_e, k = e0.numpy(), (k0 or 0)
            for s in range(2):
                if guard is None:
                    ops.sgd_flat(pa, grads[s], ba, 0.1, momentum, wd, nesterov, grad_scale=0.5)
                else:
                    ops.sgd_flat_guarded(pa, grads[s], ba, 0.1, momentum, wd, guard, nesterov, grad_scale=0.5)
                ops.sgd_flat_ema(pb, grads[s], bb, e, 0.1, momentum, wd, decay, guard=guard, nesterov=nesterov, grad_scale=0.5,
                                 warmup=warmup, updates_dev=upd)
                skipped = spec is not None and spec[1]
                if not skipped:
                    want_e = ema_update(want_e, pa.cpu().numpy(), decay, k, warmup)
                    k += 1
                ok = (_same_bits(pb, pa) and (bb is None or _same_bits(bb, ba)) and _same_bits(e, want_e)
                      and (upd is None or int(upd) == k))
                if skipped:
                    ok = ok and _same_bits(pb, p0) and (bb is None or not bool(bb.any())) and _same_bits(e, e0)
                if not ok:
                    bad.append((momentum, nesterov, wd, spec, decay, warmup, k0, s))
                    break
    assert not bad, bad


def test_a_launch_on_a_slice_leaves_the_rest_of_the_average_alone(gpu_device):
    from avid_hip import ops
    dev, N, off, n = gpu_device, 2048, 8, 1027
    full = [_rand(N, 30 + i, s) for i, s in enumerate((1.0, 0.3, 0.1, 0.01, 1.0))]
    s = slice(off, off + n)
    for optimizer in ("adam", "sgd"):
        p, g, m, v, e = (t.to(dev) for t in full)
        v.abs_()
        q, m2, v2 = p.clone(), m.clone(), v.clone()
        if optimizer == "adam":
            ops.adam_flat(q[s], g[s], m2[s], v2[s], 1e-3, 0.9, 0.999, 1e-8, 1e-5, 3)
            ops.adam_flat_ema(p[s], g[s], m[s], v[s], e[s], 1e-3, 0.9, 0.999, 1e-8, 1e-5, 3, 0.9)
            assert _same_bits(m, m2) and _same_bits(v, v2)
        else:
            ops.sgd_flat(q[s], g[s], m2[s], 0.05, 0.9, 1e-4, True)
            ops.sgd_flat_ema(p[s], g[s], m[s], e[s], 0.05, 0.9, 1e-4, 0.9, nesterov=True)
            assert _same_bits(m, m2)
        assert _same_bits(p, q) and _same_bits(g, full[1])
        assert _same_bits(e[s], ema_update(full[4][s].numpy(), q[s].cpu().numpy(), 0.9))
        assert _same_bits(e[:off], full[4][:off]) and _same_bits(e[off + n:], full[4][off + n:])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, BIG])
def test_ema_flat_is_the_restatement(gpu_device, n):
    from avid_hip import ops
    dev = gpu_device
    e0, p = _rand(n, 5), _rand(n, 6)
    pd = p.to(dev)
    for spec in GUARDS:
        for decay, warmup, k0 in (AVERAGES if n < BIG else AVERAGES[1:2]):
            guard, upd, e = _guard(dev, spec), _counter(dev, k0), e0.to(dev)
            ops.ema_flat(e, pd, decay, warmup, upd, guard)
            skipped = spec is not None and spec[1]
            want = e0.numpy() if skipped else ema_update(e0.numpy(), p.numpy(), decay, k0 or 0, warmup)
            assert _same_bits(e, want) and _same_bits(pd, p), (spec, decay, warmup, k0)
            assert upd is None or int(upd) == k0 + (0 if skipped else 1)
            if upd is not None:
                ops.ema_flat(e, pd, decay, warmup, upd, guard, advance=False)      # another reader of the same count
                assert int(upd) == k0 + (0 if skipped else 1)


SWAPS = [(n, shift) for n in (1, 3, 4, 5, 1027) for shift in ((0, 0), (1, 0), (0, 3), (2, 2))] + [(BIG, (0, 0)), (BIG, (1, 0))]


@pytest.mark.parametrize("n,shift", SWAPS)
def test_swap_flat_exchanges_and_two_exchanges_restore(gpu_device, n, shift):
    """Both pointers 16-byte aligned (vectors + tail) and every other case (the scalar path), floats ``shift`` behind a 16-byte
    boundary inside buffers whose surroundings must not change; the large size on the vector path and one scalar case."""
    from avid_hip import ops
    dev = gpu_device
    a0, b0 = _rand(n, 7), _rand(n, 8)
    wa, wb = torch.full((n + 12,), 7.0, device=dev), torch.full((n + 12,), -7.0, device=dev)
    a, b = wa[4 + shift[0]:4 + shift[0] + n], wb[4 + shift[1]:4 + shift[1] + n]
    a.copy_(a0)
    b.copy_(b0)
    ops.swap_flat(a, b)
    assert _same_bits(a, b0) and _same_bits(b, a0)
    ops.swap_flat(a, b)
    assert _same_bits(a, a0) and _same_bits(b, b0)
    for whole, s, fill in ((wa, shift[0], 7.0), (wb, shift[1], -7.0)):
        assert bool((whole[:4 + s] == fill).all()) and bool((whole[4 + s + n:] == fill).all())


def test_bad_arguments_come_back_through_the_error_convention(gpu_device):
    from avid_hip import lib, ops
    dev = gpu_device
    p, g, m, v, e = (torch.zeros(64, device=dev) for _ in range(5))
    k = torch.zeros((), dtype=torch.int64, device=dev)
    P = lambda t, byte_off=0: None if t is None else C.c_void_p(t.data_ptr() + byte_off)   # noqa: E731
    BADARG = -1
    D = lambda ema=e, decay=0.9, warmup=0, upd=None, off=0: lib.EmaDesc(None if ema is None else ema.data_ptr() + off, decay, warmup,   # noqa: E731
                                                                         None if upd is None else upd.data_ptr())
    adam, sgd = lib.raw("avid_adam_flat_ema"), lib.raw("avid_sgd_flat_ema")
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, 1.0, None)
    for what, n, ptrs, desc in (("n == 0", 0, (P(p), P(g), P(m), P(v)), D()), ("no p", 16, (None, P(g), P(m), P(v)), D()),
                                ("misaligned m", 16, (P(p), P(g), P(m, 4), P(v)), D()), ("no average", 16, (P(p), P(g), P(m), P(v)), D(None)),
                                ("misaligned average", 16, (P(p), P(g), P(m), P(v)), D(off=8)),
                                ("decay 1", 16, (P(p), P(g), P(m), P(v)), D(decay=1.0)), ("decay < 0", 16, (P(p), P(g), P(m), P(v)), D(decay=-0.5)),
                                ("warm-up without its counter", 16, (P(p), P(g), P(m), P(v)), D(warmup=1))):
        assert adam(n, *ptrs, *tail, C.byref(desc), None) == BADARG and "adam_flat_ema" in lib.last_error(), what
    assert adam(16, P(p), P(g), P(m), P(v), *tail, None, None) == BADARG
    for what, args, desc in (("n < 0", (-4, P(p), P(g), P(m)), D()), ("momentum without buf", (16, P(p), P(g), None), D()),
                             ("misaligned g", (16, P(p), P(g, 8), P(m)), D()), ("decay nan", (16, P(p), P(g), P(m)), D(decay=float("nan"))),
                             ("warm-up without its counter", (16, P(p), P(g), P(m)), D(warmup=1))):
        assert sgd(*args, 0.1, 0.9, 0.0, 0, None, 1.0, None, C.byref(desc), None) == BADARG and "sgd_flat_ema" in lib.last_error(), what
    ema, swap = lib.raw("avid_ema_flat"), lib.raw("avid_swap_flat")
    for what, args in (("n == 0", (0, P(e), P(p), 0.9, 0, None, None)), ("no e", (16, None, P(p), 0.9, 0, None, None)),
                       ("misaligned p", (16, P(e), P(p, 4), 0.9, 0, None, None)), ("decay 1", (16, P(e), P(p), 1.0, 0, None, None)),
                       ("warm-up without its counter", (16, P(e), P(p), 0.9, 1, None, None))):
        assert ema(*args, None) == BADARG and "ema_flat" in lib.last_error(), what
    for what, args in (("a == b", (16, P(p), P(p))), ("overlap", (16, P(p), P(p, 32))), ("overlap the other way", (16, P(p, 32), P(p))),
                       ("n == 0", (0, P(p), P(e))), ("no b", (16, P(p), None)), ("misaligned", (16, P(p, 2), P(e)))):
        assert swap(*args, None) == BADARG and "swap_flat" in lib.last_error(), what
    # the wrappers' own refusals
    for call in (lambda: ops.swap_flat(p, p), lambda: ops.swap_flat(p[:32], p[16:48]), lambda: ops.swap_flat(p, e[:32]),
                 lambda: ops.ema_flat(e, p, 1.0), lambda: ops.ema_flat(e, p, 0.9, True), lambda: ops.ema_flat(e, p.double(), 0.9),
                 lambda: ops.adam_flat_ema(p, g, m, v, e[::2], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.9),
                 lambda: ops.sgd_flat_ema(p, g, None, e, 0.1, 0.0, 0.0, float("nan")),
                 lambda: ops.ema_flat(e, p, 0.9, True, k.to(torch.int32))):
        with pytest.raises(lib.AvidHipError):
            call()
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in (p, g, m, v, e)) and int(k) == 0            # nothing was launched
    assert swap(16, P(p), P(p, 64), None) == 0                                        # adjacent halves do not overlap


def test_no_write_outside_the_buffers(gpu_device):
    """tests/_guards.py: every new entry point under both fills and plain at n = 1027 (vectors and a tail); no guard byte
    changes and the results are the same bits in all three runs."""
    from _guards import FILLS, guarded
    from avid_hip import ops
    dev, n = gpu_device, 1027

    def run(P):
        p, g = P(_rand(n, 40).to(dev)), P(_rand(n, 41, 0.3).to(dev))
        m, v, e = P(_rand(n, 42, 0.1).to(dev)), P(_rand(n, 43, 0.01).abs().to(dev)), P(_rand(n, 44).to(dev))
        q, buf, e2 = P(_rand(n, 45).to(dev)), P(_rand(n, 46, 0.1).to(dev)), P(_rand(n, 47).to(dev))
        k = P(torch.full((), 3, dtype=torch.int64).to(dev))
        guard = _guard(dev, (0.5, 0))
        ops.adam_flat_ema(p, g, m, v, e, 1e-3, 0.9, 0.999, 1e-8, 1e-5, 2, 0.999, warmup=True, updates_dev=k)
        ops.adam_flat_ema(p, g, m, v, e, 1e-3, 0.9, 0.999, 1e-8, 1e-5, 3, 0.999, guard=guard, warmup=True, updates_dev=k)
        ops.sgd_flat_ema(q, g, buf, e2, 0.05, 0.9, 1e-4, 0.9, nesterov=True)
        ops.sgd_flat_ema(q, g, buf, e2, 0.05, 0.9, 1e-4, 0.9, guard=guard, nesterov=True)
        ops.ema_flat(e2, p, 0.999, True, k, guard)
        ops.swap_flat(e, e2)
        ops.swap_flat(e[1:], e2[:-1])                      # the scalar path
        torch.cuda.synchronize()
        return [_bits(t) for t in (p, g, m, v, e, q, buf, e2)] + [k.cpu()]

    plain = run(lambda t: t)
    for fill in FILLS:
        with guarded(fill) as g:
            got = run(g.place)
            g.check()
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), hex(fill)


# ------------------------------------------------------------------------------------------------------------------ engines
def _snap(eng):
    torch.cuda.synchronize()
    s = {"params": eng.flat.flat.clone(), "stats": eng.flat_buffers.flat.clone()}
    if eng.m is not None:
        s.update(m=eng.m.clone(), v=eng.v.clone(), t_dev=eng.t_dev.clone())
    if eng.momentum_buffer is not None:
        s["buf"] = eng.momentum_buffer.clone()
    return s


def _assert_live_state(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert _same(a[k], b[k]), (what, k)


def _assert_average(eng, start, snaps, decay, warmup, begin=0, end=None, applied=None):
    """``ema`` / ``ema_buffers_flat`` are the restatement applied to the snapshot sequence (``applied``: which of the snapshots
    were applied steps; all of them by default) over [begin, end) and the untouched copy elsewhere; the counter counts them."""
    applied = range(len(snaps)) if applied is None else applied
    end = eng.flat.numel if end is None else end
    seq = [snaps[i] for i in applied]
    want = ema_sequence(start["params"][begin:end].cpu().numpy(), [s["params"][begin:end].cpu().numpy() for s in seq], decay, warmup)
    assert _same_bits(eng.ema[begin:end], want), "the averaged parameters"
    assert _same_bits(eng.ema[:begin], start["params"][:begin]) and _same_bits(eng.ema[end:], start["params"][end:])
    assert not _same_bits(eng.ema[begin:end], start["params"][begin:end]) and not _same_bits(eng.ema[begin:end], eng.flat.flat[begin:end])
    want = ema_sequence(start["stats"].cpu().numpy(), [s["stats"].cpu().numpy() for s in seq], decay, warmup)
    assert _same_bits(eng.ema_buffers_flat, want), "the averaged running statistics"
    assert int(eng.ema_updates) == len(seq)


def _trainstep(dev, **kw):
    import test_gpu_engine as E
    import test_gpu_plan as GP
    from avid_hip.parallel import TrainStep
    m, crit = E._model(dev), GP._crit(dev)
    return m, crit, TrainStep(m, crit, **kw)


@pytest.fixture(scope="module")
def plain_train(gpu_device):
    """Five steps of the engine as it always was (the overlapped two-slice update): the loss and the state behind each step."""
    import test_gpu_engine as E
    video, audio, ids = E._data(gpu_device, steps=5)
    m, crit, eng = _trainstep(gpu_device)
    assert eng.ema is None
    losses, states = [], []
    for i in range(5):
        losses.append(float(eng.step(video, audio, ids[i])))
        states.append(_snap(eng))
    assert eng._step_plan is not None and eng._step_plan.adam_early, "the step did not take the overlapped two-slice update"
    return losses, states


def test_trainstep_average_through_the_overlapped_update(gpu_device, plain_train):
    """Warm-up on: both slices of the overlapped update must read the same count (w = 0.9, 0.818..., ...)."""
    import test_gpu_engine as E
    video, audio, ids = E._data(gpu_device, steps=5)
    m, crit, eng = _trainstep(gpu_device, ema_decay=0.999, ema_warmup=True)
    start = _snap(eng)
    assert _same_bits(eng.ema, start["params"]) and _same_bits(eng.ema_buffers_flat, start["stats"]) and int(eng.ema_updates) == 0
    losses, states = plain_train
    snaps = []
    for i in range(4):
        assert float(eng.step(video, audio, ids[i])) == losses[i]
        snaps.append(_snap(eng))
        _assert_live_state(snaps[-1], states[i], i)
    assert eng._step_plan is not None and eng._step_plan.adam_early and 0 < eng._step_plan.adam_early < eng.flat.numel
    _assert_average(eng, start, snaps, 0.999, True)


def test_captured_graph_carries_the_average(gpu_device, plain_train):
    """Two eager steps, a capture, three replays against an eager twin: the same average, five updates counted on the device."""
    import test_gpu_engine as E
    dev = gpu_device
    video, audio, ids = E._data(dev, steps=5)
    m, c, e = _trainstep(dev, ema_decay=0.999, ema_warmup=True)
    m2, c2, twin = _trainstep(dev, ema_decay=0.999, ema_warmup=True)
    for i in range(2):
        e.step(video, audio, ids[i])
        twin.step(video, audio, ids[i])
    e.capture(video, audio, ids[2])
    torch.cuda.synchronize()
    assert e.t == 2 and int(e.ema_updates) == 2 and _same_bits(e.ema, twin.ema)      # the capture ran nothing
    for i in range(2, 5):
        e.replay(index=ids[i])
        twin.step(video, audio, ids[i])
    torch.cuda.synchronize()
    assert _same_bits(e.flat.flat, twin.flat.flat) and _same_bits(e.flat.flat, plain_train[1][4]["params"])
    assert _same_bits(e.ema, twin.ema) and _same_bits(e.ema_buffers_flat, twin.ema_buffers_flat)
    assert int(e.ema_updates) == 5 and int(twin.ema_updates) == 5 and e.t == 5


def test_trainstep_virtual_ranks_average_once_per_global_step(gpu_device):
    import test_gpu_engine as E
    video, audio, ids = E._data(gpu_device, steps=3)
    runs = []
    for kw in ({}, dict(ema_decay=0.9)):
        m, crit, eng = _trainstep(gpu_device, virtual_ranks=2, **kw)
        start, snaps, losses = _snap(eng), [], []
        for i in range(3):
            losses.append(float(eng.step(video, audio, ids[i])))
            snaps.append(_snap(eng))
        runs.append((eng, start, snaps, losses))
    (_, _, plain, plain_losses), (eng, start, snaps, losses) = runs
    assert losses == plain_losses
    for i in range(3):
        _assert_live_state(snaps[i], plain[i], i)
    _assert_average(eng, start, snaps, 0.9, False)


def test_skipped_step_leaves_the_average_alone(gpu_device):
    """skip_nonfinite, one inf in the video of the second of three steps: the average, its counter and the averaged statistics
    are those of the two applied steps; the skipped step changes none of them."""
    import test_gpu_engine as E
    video, audio, ids = E._data(gpu_device, steps=3)
    bad = video.clone()
    bad[1, 1, 3, 17, 29] = float("inf")
    m, crit, eng = _trainstep(gpu_device, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)
    start, snaps = _snap(eng), []
    for i in range(3):
        before = (eng.ema.clone(), eng.ema_buffers_flat.clone(), int(eng.ema_updates))
        eng.step(bad if i == 1 else video, audio, ids[i])
        snaps.append(_snap(eng))
        assert int(eng.guard.skipped) == (1 if i == 1 else 0)
        if i == 1:
            assert _same_bits(eng.ema, before[0]) and _same_bits(eng.ema_buffers_flat, before[1]) and int(eng.ema_updates) == before[2] == 1
            _assert_live_state(snaps[1], snaps[0], "skipped")
    assert int(eng.guard.skipped_total) == 1 and int(eng.t_dev) == 2
    _assert_average(eng, start, snaps, 0.999, True, applied=(0, 2))
    assert bool(torch.isfinite(eng.ema).all()) and bool(torch.isfinite(eng.ema_buffers_flat).all())


def _finetune_inputs(dev, steps, seed=3, bs=4):
    g = torch.Generator().manual_seed(seed)
    vids = [torch.randn((bs, 3, 8, 112, 112), generator=g).to(dev) for _ in range(steps)]
    labs = [torch.randint(0, 101, (bs,), generator=g).to(dev) for _ in range(steps)]
    return vids, labs


def _finetune(dev, **kw):
    import test_gpu_finetune as FT
    from avid_hip import parallel
    m = FT._wrapper(dev)
    m.dropout.seed, m.dropout.offset = 1234, 0
    return m, parallel.FinetuneStep(m, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(classifier_only=True), dict(optimizer="sgd", momentum=0.9, nesterov=True, weight_decay=1e-4, lr=1e-3),
                                dict(virtual_ranks=2), dict(max_grad_norm=0.05)],
                         ids=["adam", "classifier_only", "sgd", "virtual_ranks", "clipped"])
def test_finetunestep_average(gpu_device, kw):
    """Four steps with and without ``ema_decay``: the same losses, parameters, optimizer state and running statistics; the
    average is the restatement applied to the snapshots — on the classifier's slice alone under ``classifier_only``, once per
    global step under ``virtual_ranks``, through the guarded kernels with a clip that bites under ``max_grad_norm``."""
    vids, labs = _finetune_inputs(gpu_device, 4)
    runs = []
    for ema in ({}, dict(ema_decay=0.9)):
        m, eng = _finetune(gpu_device, **kw, **ema)
        start, snaps, out = _snap(eng), [], []
        for i in range(4):
            loss, hits = eng.step(vids[i], labs[i])
            out.append((float(loss), hits.tolist()))
            snaps.append(_snap(eng))
        runs.append((eng, start, snaps, out))
    (_, _, plain, plain_out), (eng, start, snaps, out) = runs
    assert out == plain_out
    for i in range(4):
        _assert_live_state(snaps[i], plain[i], i)
    if "max_grad_norm" in kw:
        assert float(eng.guard.clip_coef) < 1.0
    end = eng.n_cls if kw.get("classifier_only") else None
    _assert_average(eng, start, snaps, 0.9, False, 0, end)
    if end is not None:
        assert _same_bits(eng.ema[end:], eng.flat.flat[end:])               # the frozen tower: the copy is the live weights


def test_probestep_average(gpu_device):
    import test_gpu_probe as PR
    from avid_hip import parallel
    dev = gpu_device
    g = torch.Generator().manual_seed(9)
    vids = [torch.randn((2, 3, 8, 64, 64), generator=g).to(dev) for _ in range(4)]
    labs = [torch.randint(0, 400, (2,), generator=g).to(dev) for _ in range(4)]
    runs = []
    for ema in ({}, dict(ema_decay=0.9, ema_warmup=True)):
        eng = parallel.ProbeStep(PR._model(dev), **ema)
        start, snaps, out = _snap(eng), [], []
        for i in range(4):
            losses, hits = eng.step(vids[i], labs[i])
            out.append((losses.tolist(), hits.tolist()))
            snaps.append(_snap(eng))
        runs.append((eng, start, snaps, out))
    (_, _, plain, plain_out), (eng, start, snaps, out) = runs
    assert out == plain_out
    for i in range(4):
        _assert_live_state(snaps[i], plain[i], i)
    _assert_average(eng, start, snaps, 0.9, True)
    # the frozen tower is not in the flat buffers: the averaged model carries its live weights
    esd = eng.ema_state_dict()
    for n, p in eng.model.feature_extractor.named_parameters():
        assert _same_bits(esd["feature_extractor." + n], p), n


# ------------------------------------------------------------------------------------------------------------ ema_weights()
def test_ema_weights_make_the_model_the_averaged_one(gpu_device):
    import test_gpu_finetune as FT
    from avid_hip import parallel
    dev = gpu_device
    vids, labs = _finetune_inputs(dev, 3, seed=5, bs=2)
    g = torch.Generator().manual_seed(6)
    V, clips = 2, 2
    video = torch.randn((V, clips, 3, 8, 112, 112), generator=g).to(dev)
    labels = torch.randint(0, 101, (V,), generator=g).to(dev)
    x = video.flatten(0, 1).contiguous()
    m, eng = _finetune(dev, ema_decay=0.9)
    m2, twin = _finetune(dev, ema_decay=0.9)                 # never enters the block
    for i in range(2):
        eng.step(vids[i], labs[i])
        twin.step(vids[i], labs[i])
    # the reference: a fresh model loaded from ema_state_dict()
    fresh = FT._wrapper(dev, seed=1)
    fresh.load_state_dict(eng.ema_state_dict(), strict=True)
    want_eval = parallel.FinetuneStep(fresh).evaluate(video, labels, 2)
    want_infer = parallel.Inference(fresh)(x)
    fresh.eval()
    with torch.no_grad():
        want_layers = fresh(x)
    live = _snap(eng)
    live_out = parallel.Inference(m)(x)
    assert not _same_bits(live_out, want_infer)
    names = dict(m.named_parameters())
    versions = {n: p._version for n, p in names.items()}
    with eng.ema_weights() as inside:
        assert inside is eng
        infer = parallel.Inference(m)
        assert _same_bits(infer(x), want_infer) and infer.used_programs
        got = eng.evaluate(video, labels, 2)
        assert all(_same(a, b) for a, b in zip(got, want_eval))
        m.eval()
        with torch.no_grad():
            assert _same_bits(m(x), want_layers)
        m.train()
        assert all(p._version > versions[n] for n, p in names.items())
        sd = m.state_dict()
        assert all(_same(sd[k], v) for k, v in fresh.state_dict().items())
        for call in (lambda: eng.step(vids[2], labs[2]), eng.state_dict, eng.ema_state_dict, eng.ema_reset,
                     lambda: eng.ema_weights().__enter__()):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()
        assert eng.t == 2 and m.dropout.offset == m2.dropout.offset
    _assert_live_state(_snap(eng), live, "after the block")
    assert _same_bits(parallel.Inference(m)(x), live_out) and _same_bits(eng.ema, twin.ema)
    # an exception inside the block: the exchange is undone
    with pytest.raises(KeyError):
        with eng.ema_weights():
            raise KeyError("inside")
    _assert_live_state(_snap(eng), live, "after an exception")
    assert not eng._ema_swapped
    la, ha = eng.step(vids[2], labs[2])
    lb, hb = twin.step(vids[2], labs[2])
    assert float(la) == float(lb) and torch.equal(ha, hb)
    _assert_live_state(_snap(eng), _snap(twin), "the step after the block")
    assert _same_bits(eng.ema, twin.ema) and _same_bits(eng.ema_buffers_flat, twin.ema_buffers_flat)


def test_ema_weights_with_live_statistics(gpu_device):
    """``ema_buffers=False``: inside the block the parameters are the averaged ones, the running statistics the live ones."""
    dev = gpu_device
    vids, labs = _finetune_inputs(dev, 2, seed=7, bs=2)
    m, eng = _finetune(dev, ema_decay=0.9, ema_buffers=False)
    assert eng.ema_buffers_flat is None
    for i in range(2):
        eng.step(vids[i], labs[i])
    live = _snap(eng)
    with eng.ema_weights():
        assert _same_bits(eng.flat_buffers.flat, live["stats"]) and _same_bits(eng.ema, live["params"])
        assert not _same_bits(eng.flat.flat, live["params"])
    _assert_live_state(_snap(eng), live, "after the block")


# -------------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_resumes_the_average_bit_for_bit(gpu_device):
    import test_gpu_finetune as FT
    from avid_hip import parallel
    dev = gpu_device
    vids, labs = _finetune_inputs(dev, 4, seed=8, bs=2)
    kw = dict(ema_decay=0.999, ema_warmup=True)
    m, eng = _finetune(dev, **kw)
    for i in range(4):
        eng.step(vids[i], labs[i])
    want = _snap(eng)
    m1, first = _finetune(dev, **kw)
    for i in range(2):
        first.step(vids[i], labs[i])
    torch.cuda.synchronize()
    msd = {k: v.clone() for k, v in m1.state_dict().items()}
    osd = copy.deepcopy(first.state_dict())
    assert osd["avid_ema"]["num_updates"] == 2 and sorted(osd["avid_ema"]["params"]) == list(range(len(list(m1.parameters()))))
    m2 = FT._wrapper(dev, seed=1)
    m2.load_state_dict(msd)
    m2.dropout.seed, m2.dropout.offset = m1.dropout.seed, m1.dropout.offset
    second = parallel.FinetuneStep(m2, ema_decay=0.5)
    second.load_state_dict(osd)
    assert (second.ema_decay, second.ema_warmup, int(second.ema_updates)) == (0.999, True, 2)
    for i in range(2, 4):
        second.step(vids[i], labs[i])
    _assert_live_state(_snap(second), want, "resumed")
    assert _same_bits(second.ema, eng.ema) and _same_bits(second.ema_buffers_flat, eng.ema_buffers_flat)
    assert int(second.ema_updates) == int(eng.ema_updates) == 4
    # a checkpoint without an average: the engine keeps its own and says so; ema_reset() restarts it from the weights
    with pytest.warns(UserWarning, match="no weight average"):
        second.load_state_dict(parallel.FinetuneStep(FT._wrapper(dev, seed=2)).state_dict())
    assert _same_bits(second.ema, eng.ema)
    second.ema_reset()
    assert _same_bits(second.ema, second.flat.flat) and _same_bits(second.ema_buffers_flat, second.flat_buffers.flat) and int(second.ema_updates) == 0
