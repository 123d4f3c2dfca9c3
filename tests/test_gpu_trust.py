"""Per-tensor hyper-parameters and LARS / LAMB on a real MI355X: the per-segment norms against ``math.fsum``, the table-driven
kernels against the existing flat kernels bit for bit, LARS against the float32 restatement bit for bit, LAMB inside the derived
bound of float64 (tests/_trust_ref.py), guard, average, error convention, guard bands, and the three step engines.

The table of the kernel tests has segment lengths 1, 3, 4, 5, 64, 1027, one chunk exactly (4096), one chunk + 1 and BIG — with
it the buffer holds 1034 chunks, more than the 4 x 256 workgroups a launch gets: the chunk loop's second round — laid out with
``FlatParams``' padding (every segment starts on a multiple of 4 floats)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _trust_ref as R
from _ema_ref import ema_update

pytestmark = pytest.mark.gpu

BIG = 4 * 256 * 4096 + 7
NUMELS = [1, 3, 4, 5, 64, 1027, 4096, 4097, BIG]
SCALES = [1.0, 0.5, 0.125, 2.0, 1.0, 0.25, 0.75, 0.5, 0.3]
DECAYS = [0.0, 1e-4, 1e-4, 0.0, 5e-4, 1e-4, 0.0, 1e-4, 1e-4]
ADAPT = [True, True, False, True, True, True, True, True, True]


def _bits(t):
    t = torch.from_numpy(t) if isinstance(t, np.ndarray) else t.detach().cpu()
    return t.contiguous().view(torch.int32)


def _same_bits(got, want):
    return torch.equal(_bits(got), _bits(want))


def _table(dev, scales=1.0, decays=0.0, adapt=True, numels=NUMELS):
    from avid_hip import ops
    segs, n = R.padded_table(numels, scales, decays, adapt)
    tab = ops.SegmentTable([(s.offset, s.numel) for s in segs], [s.lr_scale for s in segs], [s.weight_decay for s in segs],
                           [s.adapt for s in segs], device=dev, numel=n)
    return segs, n, tab


def _fill(segs, n, seed, scale=1.0, pad=0.0, zero=()):
    """float32 [n]: normal numbers inside the segments (zeros in the segments listed in ``zero``), ``pad`` on the padding lanes."""
    x = (scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))).numpy()
    x[R.padding_mask(segs, n)] = pad
    for k in zero:
        x[segs[k].offset:segs[k].offset + segs[k].numel] = 0.0
    return x


def _lr32(lr, scale):
    return float(np.float32(lr) * np.float32(scale))


# -------------------------------------------------------------------------------------------------------------------- norms
def test_segment_norms_are_fsum_to_an_ulp_and_deterministic(gpu_device):
    """Every segment's sum of squares, rounded to float32, within 1 ulp of the ``fsum`` value; the same bits on a second run and
    under 8 and 24 reserved CUs; padding lanes holding 1e30 enter no sum and are not written."""
    from avid_hip import ops
    dev = gpu_device
    segs, n, tab = _table(dev)
    x, y = _fill(segs, n, 1, pad=1e30), _fill(segs, n, 2, 0.3, pad=1e30)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    sums = ops.segment_sumsq(tab, xd, yd)
    got = sums.cpu().numpy()
    want = np.array([R.segment_sumsq(x, segs), R.segment_sumsq(y, segs)]).T
    worst = 0.0
    for s in range(len(segs)):
        for c in range(2):
            g32, w32 = np.float32(got[s, c]), np.float32(want[s, c])
            assert abs(float(g32) - float(w32)) <= float(np.spacing(w32)), (s, c, got[s, c], want[s, c])
            worst = max(worst, abs(got[s, c] - want[s, c]) / want[s, c])
    print(f"\n[segment norms] worst relative distance of the double sums from fsum: {worst:.2e}")
    assert worst < 1e-12                                   # (what double accumulation leaves: far inside the float32 ulp)
    assert torch.equal(ops.segment_sumsq(tab, xd, yd).view(torch.int64), sums.view(torch.int64))
    full = ops.cu_budget()
    try:
        for reserve in (8, 24):
            assert ops.set_cu_budget(full - reserve) == full - reserve
            assert torch.equal(ops.segment_sumsq(tab, xd, yd).view(torch.int64), sums.view(torch.int64)), reserve
    finally:
        ops.set_cu_budget(0)
    one = ops.segment_sumsq(tab, xd)
    assert torch.equal(one[:, 0].view(torch.int64), sums[:, 0].view(torch.int64)) and not one[:, 1].any()
    assert _same_bits(xd, x) and _same_bits(yd, y)


def test_padding_lanes_are_neither_read_into_a_norm_nor_written(gpu_device):
    """p and g with 1e30 on every padding lane through LARS and LAMB: the factors are those of zero padding, and the padding of
    p, of the state and of the average holds what it held."""
    from avid_hip import ops
    dev = gpu_device
    segs, n, tab = _table(dev, SCALES, DECAYS, ADAPT)
    pad = torch.from_numpy(R.padding_mask(segs, n)).to(dev)
    out = {}
    for fill in (0.0, 1e30):
        p = torch.from_numpy(_fill(segs, n, 3, pad=fill)).to(dev)
        g = torch.from_numpy(_fill(segs, n, 4, 0.3, pad=fill)).to(dev)
        buf, e = torch.full((n,), 5.0, device=dev), torch.full((n,), 6.0, device=dev)
        ops.sgd_flat_table(tab, p, g, buf, 0.1, 0.9, True, trust_coefficient=0.001, ema=e, decay=0.9)
        q = tab.trust.clone()
        p2 = torch.from_numpy(_fill(segs, n, 3, pad=fill)).to(dev)
        m, v = torch.full((n,), 7.0, device=dev), torch.full((n,), 8.0, device=dev)
        ops.lamb_flat(tab, p2, g, m, v, 1e-2, 0.9, 0.999, 1e-6, 1)
        r = tab.trust.clone()
        for t, was in ((p, fill), (p2, fill), (g, fill), (buf, 5.0), (e, 6.0), (m, 7.0), (v, 8.0)):
            assert bool((t[pad] == was).all())
        out[fill] = (q, r, p[~pad].clone(), p2[~pad].clone())
    for a, b in zip(out[0.0], out[1e30]):
        assert _same_bits(a, b)


# ---------------------------------------------------------------------------------- grouped kernels against the existing ones
@pytest.mark.parametrize("words", ["by_value", "lr_dev", "lr_dev+step_dev"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_adam_flat_table_has_the_bits_of_adam_flat(gpu_device, grad_scale, words):
    """Three steps.  A uniform table: ``ops.adam_flat`` over the same whole buffers.  A mixed table: ``ops.adam_flat`` called once per
    segment with that segment's values, lr as the float32 product.  ``adam_flat``'s own n % 4 tail is contracted differently
    from its 16-byte vector loop by the compiler (csrc/optim.hip: adam_element), a flat buffer laid out by ``FlatParams`` has no
    such tail, and the table kernel computes every element as the vector loop does — so the per-segment reference calls run over
    the segment's padded extent, whose padding lanes are zero in p, g, m and v and stay zero."""
    from avid_hip import ops
    dev, lr, b1, b2, eps = gpu_device, 1e-3, 0.9, 0.999, 1e-8
    for scales, decays in ((1.0, 1e-4), (SCALES, DECAYS)):
        segs, n, tab = _table(dev, scales, decays)
        p = torch.from_numpy(_fill(segs, n, 5)).to(dev)
        rp = p.clone()
        m, v, rm, rv = (torch.zeros(n, device=dev) for _ in range(4))
        lr_dev = torch.full((), lr, dtype=torch.float32, device=dev) if words != "by_value" else None
        t_dev, rt_dev = ((torch.zeros((), dtype=torch.int64, device=dev) for _ in range(2)) if words.endswith("step_dev")
                         else (None, None))
        seg_lr = [torch.full((), _lr32(lr, s.lr_scale), dtype=torch.float32, device=dev) for s in segs] if lr_dev is not None else None
        host_lr = 123.0 if lr_dev is not None else lr                 # with lr_dev the host's value is wrong and not used
        for step in range(1, 4):
            g = torch.from_numpy(_fill(segs, n, 10 + step, 0.3)).to(dev)
            ops.adam_flat_table(tab, p, g, m, v, host_lr, b1, b2, eps, step, grad_scale=grad_scale, step_dev=t_dev, lr_dev=lr_dev)
            if scales == 1.0:
                ops.adam_flat(rp, g, rm, rv, host_lr, b1, b2, eps, decays, step, grad_scale=grad_scale, step_dev=rt_dev,
                              lr_dev=lr_dev)
            else:
                for k, s in enumerate(segs):
                    sl = slice(s.offset, s.offset + (s.numel + 3) // 4 * 4)
                    ops.adam_flat(rp[sl], g[sl], rm[sl], rv[sl], 123.0 if seg_lr else _lr32(lr, s.lr_scale), b1, b2, eps,
                                  s.weight_decay, step, grad_scale=grad_scale, step_dev=rt_dev,
                                  lr_dev=seg_lr[k] if seg_lr else None, advance=k == 0)
            assert _same_bits(p, rp) and _same_bits(m, rm) and _same_bits(v, rv), (scales == 1.0, step)
        assert t_dev is None or int(t_dev) == int(rt_dev) == 3
        assert not bool(torch.isnan(p).any()) and not _same_bits(p, torch.from_numpy(_fill(segs, n, 5)))


@pytest.mark.parametrize("words", ["by_value", "lr_dev"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_sgd_flat_table_has_the_bits_of_sgd_flat(gpu_device, grad_scale, words):
    """As above for the SGD family (there is no step counter), over {no momentum, momentum, Nesterov}; the per-segment reference
    calls take the segment exactly."""
    from avid_hip import ops
    dev, lr = gpu_device, 0.1
    for scales, decays in ((1.0, 1e-4), (SCALES, DECAYS)):
        segs, n, tab = _table(dev, scales, decays)
        lr_dev = torch.full((), lr, dtype=torch.float32, device=dev) if words == "lr_dev" else None
        seg_lr = [torch.full((), _lr32(lr, s.lr_scale), dtype=torch.float32, device=dev) for s in segs] if lr_dev is not None else None
        host_lr = 123.0 if lr_dev is not None else lr
        for momentum, nesterov in ((0.0, False), (0.9, False), (0.9, True)):
            p = torch.from_numpy(_fill(segs, n, 6)).to(dev)
            rp = p.clone()
            buf, rbuf = (torch.zeros(n, device=dev), torch.zeros(n, device=dev)) if momentum else (None, None)
            for step in range(3):
                g = torch.from_numpy(_fill(segs, n, 20 + step, 0.3)).to(dev)
                ops.sgd_flat_table(tab, p, g, buf, host_lr, momentum, nesterov, grad_scale=grad_scale, lr_dev=lr_dev)
                if scales == 1.0:
                    ops.sgd_flat(rp, g, rbuf, host_lr, momentum, decays, nesterov, grad_scale=grad_scale, lr_dev=lr_dev)
                else:
                    for k, s in enumerate(segs):
                        sl = slice(s.offset, s.offset + s.numel)
                        ops.sgd_flat(rp[sl], g[sl], None if rbuf is None else rbuf[sl], 123.0 if seg_lr else _lr32(lr, s.lr_scale),
                                     momentum, s.weight_decay, nesterov, grad_scale=grad_scale, lr_dev=seg_lr[k] if seg_lr else None)
                assert _same_bits(p, rp) and (buf is None or _same_bits(buf, rbuf)), (scales == 1.0, momentum, nesterov, step)
            assert not bool(torch.isnan(p).any())


# --------------------------------------------------------------------------------------------------------------------- LARS
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_lars_is_the_float32_restatement(gpu_device, nesterov, wd):
    """Three steps, momentum 0.9, grad_scale 0.5.  Every segment's q, read from the trust array, within 1 ulp of the restatement's
    (``fsum`` norms); p and buf bit for bit the float32 restatement evaluated with the ``fsum``-derived q.  Segment 2 is not
    adapted, segment 3 starts with all-zero parameters and segment 4 has an all-zero gradient (q = 1).  Seeds 30.. : no q of
    these runs sits on a rounding tie (the bit comparison of p would say so)."""
    from avid_hip import ops
    dev, eta, lr, gs = gpu_device, 0.001, 0.1, 0.5
    decays = [wd if d else 0.0 for d in DECAYS]
    segs, n, tab = _table(dev, SCALES, decays, ADAPT)
    p = _fill(segs, n, 30, zero=(3,))
    buf = np.zeros(n, np.float32)
    pd, bd = torch.from_numpy(p).to(dev), torch.zeros(n, device=dev)
    for step in range(3):
        g = _fill(segs, n, 31 + step, 0.3, zero=(4,))
        gd = torch.from_numpy(g).to(dev)
        ops.sgd_flat_table(tab, pd, gd, bd, lr, 0.9, nesterov, grad_scale=gs, trust_coefficient=eta)
        q = R.lars_q(p, g, segs, eta, gs)
        got = tab.trust.cpu().numpy()
        for k in range(len(segs)):
            assert abs(float(got[k]) - float(q[k])) <= float(np.spacing(np.float32(q[k]))), (step, k, got[k], q[k])
        assert got[2] == 1.0 and (step > 0 or got[3] == 1.0) and (wd != 0 or got[4] == 1.0) and got[0] != 1.0 and got[8] != 1.0
        p, buf = R.grouped_sgd_step(p, g, buf, segs, lr, 0.9, nesterov, gs, q=q)
        assert _same_bits(pd, p), ("parameters", step)
        assert _same_bits(bd, buf), ("momentum buffer", step)
        assert _same_bits(gd, g)
    assert not np.isnan(p).any()


def test_lars_without_an_adapted_segment_is_sgd_flat_table(gpu_device):
    from avid_hip import ops
    dev = gpu_device
    segs, n, tab = _table(dev, SCALES, DECAYS, False)
    p = torch.from_numpy(_fill(segs, n, 40)).to(dev)
    rp = p.clone()
    buf, rbuf = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step in range(3):
        g = torch.from_numpy(_fill(segs, n, 41 + step, 0.3)).to(dev)
        ops.sgd_flat_table(tab, p, g, buf, 0.1, 0.9, True, grad_scale=0.5, trust_coefficient=0.001)
        assert bool((tab.trust == 1.0).all())
        ops.sgd_flat_table(tab, rp, g, rbuf, 0.1, 0.9, True, grad_scale=0.5)
        assert _same_bits(p, rp) and _same_bits(buf, rbuf), step


# --------------------------------------------------------------------------------------------------------------------- LAMB
def test_lamb_is_inside_the_bound_of_float64(gpu_device):
    """Three steps, grad_scale 0.5: p, m and v within ``_trust_ref.LambBound`` of the float64 yardstick in every element, the
    ratios within 1e-5 of its ratios (a sanity check: the bound on p is what holds them); m and v the bits ``ops.adam_flat(weight_decay=0)`` leaves."""
    from avid_hip import ops
    dev, lr, b1, b2, eps, gs = gpu_device, 1e-2, 0.9, 0.999, 1e-6, 0.5
    decays = [1e-2 if d else 0.0 for d in DECAYS]
    segs, n, tab = _table(dev, SCALES, decays, ADAPT)
    p0 = _fill(segs, n, 50, zero=(3,))
    pd = torch.from_numpy(p0).to(dev)
    md, vd, am, av = (torch.zeros(n, device=dev) for _ in range(4))
    ap = pd.clone()
    bound = R.LambBound(n)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    mask = ~R.padding_mask(segs, n)
    worst = {}
    for step in range(1, 4):
        g = _fill(segs, n, 50 + step, 0.3, zero=(4,))
        gd = torch.from_numpy(g).to(dev)
        ops.lamb_flat(tab, pd, gd, md, vd, lr, b1, b2, eps, step, grad_scale=gs)
        ops.adam_flat(ap, gd, am, av, lr, b1, b2, eps, 0.0, step, grad_scale=gs)
        assert _same_bits(md, am) and _same_bits(vd, av), step
        assert _same_bits(gd, g)
        _, _, _, r64 = R.lamb_step(p64, g.astype(np.float64), m64, v64, segs, lr, b1, b2, eps, step, gs, dtype=np.float64)
        p64, m64, v64 = bound.step(p64, g.astype(np.float64), m64, v64, segs, lr, b1, b2, eps, step, gs)
        np.testing.assert_allclose(tab.trust.cpu().numpy(), np.array(r64, np.float64), rtol=1e-5)
        for name, got, ref, e in (("p", pd, p64, bound.ep), ("m", md, m64, bound.em), ("v", vd, v64, bound.ev)):
            ratio = np.abs(got.cpu().numpy().astype(np.float64) - ref)[mask] / np.maximum(e[mask], 1e-300)
            worst[(name, step)] = float(ratio.max())
    print(f"\n[lamb] worst |kernel - float64| / bound per buffer and step: {worst}")
    assert max(worst.values()) <= 1.0, worst
    r = tab.trust.cpu().numpy()
    assert r[2] == 1.0 and r[0] != 1.0 and r[8] != 1.0


# ------------------------------------------------------------------------------------------------------- guard and average
def _families(dev, tab, n):
    """name -> (state tensors, run(p, g, state, **kw)) for the three table-driven updates."""
    from avid_hip import ops
    z = lambda: torch.zeros(n, device=dev)      # noqa: E731
    return {
        "lars": (lambda: [z()], lambda p, g, st, **kw: ops.sgd_flat_table(tab, p, g, st[0], 0.1, 0.9, True, grad_scale=0.5,
                                                                          trust_coefficient=0.001, **kw)),
        "adam": (lambda: [z(), z()], lambda p, g, st, **kw: ops.adam_flat_table(tab, p, g, st[0], st[1], 1e-3, 0.9, 0.999, 1e-8, 1,
                                                                                grad_scale=0.5, **kw)),
        "lamb": (lambda: [z(), z()], lambda p, g, st, **kw: ops.lamb_flat(tab, p, g, st[0], st[1], 1e-2, 0.9, 0.999, 1e-6, 1,
                                                                          grad_scale=0.5, **kw)),
    }


@pytest.mark.parametrize("family", ["lars", "adam", "lamb"])
def test_guard_record_and_average(gpu_device, family):
    """skip = 1: nothing changes — p, the state, the average, the trust array, the device step counter.  clip_coef = 0.25: the
    unguarded kernel fed 0.25 g (exactly scaled), bit for bit, trust array included.  With an average: ``ops.ema_flat`` applied
    behind the plain kernel, bit for bit (what tests/test_gpu_ema.py asks of the fused Adam)."""
    from avid_hip import ops
    dev = gpu_device
    segs, n, tab = _table(dev, SCALES, DECAYS, ADAPT)
    make, run = _families(dev, tab, n)[family]
    p0 = torch.from_numpy(_fill(segs, n, 60)).to(dev)
    g = torch.from_numpy(_fill(segs, n, 61, 0.3)).to(dev)
    e0 = torch.from_numpy(_fill(segs, n, 62)).to(dev)
    guard = ops.StepGuard(dev)
    # a skipped step
    guard.clip_coef.fill_(1.0)
    guard.skipped.fill_(1)
    p, st, e = p0.clone(), make(), e0.clone()
    tab.trust.fill_(7.0)
    run(p, g, st, guard=guard, ema=e, decay=0.9)
    assert _same_bits(p, p0) and all(not bool(s.any()) for s in st) and _same_bits(e, e0) and bool((tab.trust == 7.0).all())
    if family != "lars":
        t_dev = torch.full((), 4, dtype=torch.int64, device=dev)
        run(p, g, st, guard=guard, step_dev=t_dev)
        assert int(t_dev) == 4 and _same_bits(p, p0) and all(not bool(s.any()) for s in st)
    # a clipped step
    guard.skipped.fill_(0)
    guard.clip_coef.fill_(0.25)
    run(p, g, st, guard=guard)
    clipped_trust = tab.trust.clone()
    rp, rst = p0.clone(), make()
    run(rp, 0.25 * g, rst)
    assert _same_bits(p, rp) and all(_same_bits(a, b) for a, b in zip(st, rst)) and _same_bits(clipped_trust, tab.trust)
    assert not _same_bits(p, p0)
    # an unclipped guarded step is the unguarded one
    guard.clip_coef.fill_(1.0)
    p, st = p0.clone(), make()
    run(p, g, st, guard=guard)
    rp, rst = p0.clone(), make()
    run(rp, g, rst)
    assert _same_bits(p, rp) and all(_same_bits(a, b) for a, b in zip(st, rst))
    # the average, with and without the guard, warm-up count 3
    k = torch.full((), 3, dtype=torch.int64, device=dev)
    for gd in (None, guard):
        k.fill_(3)
        p, st, e = p0.clone(), make(), e0.clone()
        run(p, g, st, guard=gd, ema=e, decay=0.999, warmup=True, updates_dev=k)
        assert int(k) == 4
        assert _same_bits(p, rp) and all(_same_bits(a, b) for a, b in zip(st, rst))
        k.fill_(3)
        want = e0.clone()
        ops.ema_flat(want, rp, 0.999, True, k)
        assert _same_bits(e, want)
        seg = segs[5]
        sl = slice(seg.offset, seg.offset + seg.numel)
        assert _same_bits(e[sl], ema_update(e0[sl].cpu().numpy(), rp[sl].cpu().numpy(), 0.999, 3, True))


# --------------------------------------------------------------------------------------------------------- error convention
def test_bad_tables_come_back_through_the_error_convention(gpu_device):
    from avid_hip import lib, ops
    dev = gpu_device
    segs, n, tab = _table(dev, numels=[5, 64, 4097])
    p, g, m, v = (torch.zeros(n, device=dev) for _ in range(4))
    trust, sums = torch.zeros(3, device=dev), torch.zeros(6, dtype=torch.float64, device=dev)
    ws = torch.zeros(tab.workspace_bytes(), dtype=torch.uint8, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    BADARG = -1

    def broken(change):
        host = (lib.Segment * tab.S)(*[lib.Segment(s.offset, s.numel, s.lr_scale, s.weight_decay, s.adapt, s.first_chunk)
                                       for s in tab.segs])
        change(host)
        d = lib.SegmentTable(tab.S, tab.n_chunks, C.addressof(host), tab.seg_dev.data_ptr(), C.addressof(tab.chunks),
                             tab.chunk_dev.data_ptr())
        return d, host

    def setter(k, field, value):
        return lambda host: setattr(host[k], field, value)
    cases = {"aligned": setter(1, "offset", 10), "increasing": setter(2, "offset", 0), "exceeds n": setter(2, "numel", 5000),
             "finite": setter(0, "lr_scale", float("nan")), "not finite": setter(1, "weight_decay", float("inf")),
             "overlapping": setter(1, "offset", 4), "adapt": setter(0, "adapt", 3)}
    for word, change in cases.items():
        d, host = broken(change)
        t = C.byref(d)
        calls = {"segment_sumsq": lambda: lib.raw("avid_segment_sumsq")(t, n, P(p), None, P(sums), None, P(ws), ws.numel(), None),
                 "sgd_flat_table": lambda: lib.raw("avid_sgd_flat_table")(t, n, P(p), P(g), None, 0.1, 0.0, 0, None, 1.0, 0.001, P(trust),
                                                                          None, None, P(ws), ws.numel(), None),
                 "adam_flat_table": lambda: lib.raw("avid_adam_flat_table")(t, n, P(p), P(g), P(m), P(v), 1e-3, 0.9, 0.999, 1e-8, 1,
                                                                            None, None, 1.0, None, None, None),
                 "lamb_flat": lambda: lib.raw("avid_lamb_flat")(t, n, P(p), P(g), P(m), P(v), 1e-3, 0.9, 0.999, 1e-8, 1, None, None,
                                                                 1.0, P(trust), None, None, P(ws), ws.numel(), None)}
        for name, call in calls.items():
            assert call() == BADARG and name in lib.last_error() and word in lib.last_error(), (name, word, lib.last_error())
    with pytest.raises(lib.AvidHipError, match="sgd_flat_table"):
        ops.sgd_flat_table(tab, p, g, None, 0.1, 0.9)                       # momentum without its buffer
    with pytest.raises(lib.AvidHipError, match="buffer of"):
        ops.adam_flat_table(tab, p[:8], g[:8], m[:8], v[:8], 1e-3, 0.9, 0.999, 1e-8, 1)
    torch.cuda.synchronize()
    g.fill_(1.0)
    for t_ in (p, m, v, trust, sums):
        assert not bool(t_.any())                                           # nothing was launched
    ops.adam_flat_table(tab, p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1)         # ... and the good table runs
    assert bool(p.any())


# --------------------------------------------------------------------------------------------------------------- guard bands
def test_no_write_outside_the_buffers(gpu_device):
    """tests/_guards.py: every new op between guard bands under both fills, workspaces of exactly the size the query returns,
    the table's device copies and the trust array guarded too; no band byte changes and the results are the plain run's bits."""
    from _guards import FILLS, guarded
    from avid_hip import ops
    dev = gpu_device

    def run(place):
        segs, n, tab = _table(dev, SCALES, DECAYS, ADAPT)
        new = lambda seed, scale=1.0: place(torch.from_numpy(_fill(segs, n, seed, scale)).to(dev))      # noqa: E731
        g = new(71, 0.3)
        sums = ops.segment_sumsq(tab, new(70), g)
        p1, b1, e1 = new(70), new(72, 0.1), new(73)
        ops.sgd_flat_table(tab, p1, g, b1, 0.1, 0.9, True, grad_scale=0.5, trust_coefficient=0.001, ema=e1, decay=0.9)
        q = tab.trust.clone()
        p2, m2, v2 = new(70), new(74, 0.01), new(75, 0.01).abs()
        ops.adam_flat_table(tab, p2, g, m2, v2, 1e-3, 0.9, 0.999, 1e-8, 2, grad_scale=0.5)
        p3, m3, v3, e3 = new(70), new(74, 0.01), new(75, 0.01).abs(), new(73)
        ops.lamb_flat(tab, p3, g, m3, v3, 1e-2, 0.9, 0.999, 1e-6, 2, grad_scale=0.5, ema=e3, decay=0.9)
        torch.cuda.synchronize()
        return [_bits(t) for t in (sums.view(torch.int64).view(torch.float32), p1, b1, e1, q, p2, m2, v2, p3, m3, v3, e3, tab.trust, g)]

    plain = run(lambda t: t)
    for fill in FILLS:
        with guarded(fill) as gd:
            got = run(gd.place)
            gd.check()
        assert gd.workspaces and all(nbytes == 1034 * 16 for nbytes, *_ in gd.workspaces), gd.workspaces
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), hex(fill)


# ------------------------------------------------------------------------------------------------------------------ engines
def _finetune_inputs(dev, steps, seed=3, batch=4):
    g = torch.Generator().manual_seed(seed)
    vids = [torch.randn((batch, 3, 8, 112, 112), generator=g).to(dev) for _ in range(steps)]
    labs = [torch.randint(0, 101, (batch,), generator=g).to(dev) for _ in range(steps)]
    return vids, labs


def _probe_inputs(dev, steps, seed=9):
    g = torch.Generator().manual_seed(seed)
    vids = [torch.randn((2, 3, 8, 64, 64), generator=g).to(dev) for _ in range(steps)]
    labs = [torch.randint(0, 400, (2,), generator=g).to(dev) for _ in range(steps)]
    return vids, labs


def _tower_rules(m):
    """The tower at lr_scale 0.125, 1-d tensors undecayed and not adapted (the first match wins: one rule per tensor)."""
    rules = []
    for n, p in m.named_parameters():
        d = {}
        if n.startswith("feature_extractor."):
            d["lr_scale"] = 0.125
        if p.ndim <= 1:
            d.update(weight_decay=0.0, adapt=False)
        if d:
            rules.append(("^" + n.replace(".", r"\.") + "$", d))
    return rules


def _fresh_table(eng):
    """An ``ops.SegmentTable`` of the engine's values over the slice it updates, built here (not the engine's own object)."""
    from avid_hip import ops
    vals = eng.param_values()
    begin, end = eng._update_range()
    return ops.SegmentTable(eng.flat, [v[1] for v in vals], [v[2] for v in vals], [v[3] for v in vals], begin=begin, end=end), begin, end


def _snapshot(eng):
    keep = {"p": eng.flat.flat.clone()}
    for name in ("momentum_buffer", "m", "v", "t_dev"):
        t = getattr(eng, name)
        if t is not None:
            keep[name] = t.clone()
    return keep


def _op_on_snapshot(eng, snap, grad_scale=1.0):
    """The op-level call of the engine's optimizer on ``snap`` (clones from before the step) with the gradient the step left;
    returns the table it used."""
    from avid_hip import ops
    tab, b, e = _fresh_table(eng)
    g = eng.flat.grad[b:e]
    if eng.optimizer in ("sgd", "lars"):
        buf = snap.get("momentum_buffer")
        ops.sgd_flat_table(tab, snap["p"][b:e], g, None if buf is None else buf[b:e], eng.lr, eng.momentum, eng.nesterov,
                           grad_scale=grad_scale, trust_coefficient=eng.trust_coefficient if eng.optimizer == "lars" else None)
    else:
        fn = ops.lamb_flat if eng.optimizer == "lamb" else ops.adam_flat_table
        fn(tab, snap["p"][b:e], g, snap["m"][b:e], snap["v"][b:e], eng.lr, eng.betas[0], eng.betas[1], eng.eps, 0,
           grad_scale=grad_scale, step_dev=snap["t_dev"])
    return tab


def _assert_engine_is(eng, snap, tab=None):
    for name, want in snap.items():
        got = eng.flat.flat if name == "p" else getattr(eng, name)
        assert torch.equal(got, want) if name == "t_dev" else _same_bits(got, want), name
    if tab is not None and eng.optimizer in ("lars", "lamb"):
        assert _same_bits(eng.trust, tab.trust) and not bool((eng.trust == 1.0).all())


def test_finetune_sgd_with_rules_is_sgd_flat_table(gpu_device):
    import test_gpu_finetune as FT
    from avid_hip import parallel
    dev = gpu_device
    vids, labs = _finetune_inputs(dev, 1)
    m = FT._wrapper(dev)
    eng = parallel.FinetuneStep(m, lr=1e-3, optimizer="sgd", momentum=0.9, nesterov=True, weight_decay=1e-4,
                                param_rules=_tower_rules(m))
    vals = {n: (s, w, a) for n, s, w, a in eng.param_values()}
    assert vals["classifier.weight"] == (1.0, 1e-4, True) and vals["classifier.bias"] == (1.0, 0.0, False)
    assert vals["feature_extractor.conv1.0.weight"] == (0.125, 1e-4, True)
    assert sum(1 for s, w, a in vals.values() if w == 0.0) == sum(1 for p in m.parameters() if p.ndim <= 1) > 10
    from avid_hip import ops
    snap, uniform = _snapshot(eng), _snapshot(eng)
    eng.step(vids[0], labs[0])
    torch.cuda.synchronize()
    assert bool(eng.flat.grad.any())
    _op_on_snapshot(eng, snap)
    _assert_engine_is(eng, snap)
    # ... which is not what the engine's base values alone give: the tower moved less
    ops.sgd_flat(uniform["p"], eng.flat.grad, uniform["momentum_buffer"], 1e-3, 0.9, 1e-4, True)
    assert not _same_bits(uniform["p"][eng.n_cls:], eng.flat.flat[eng.n_cls:])


def test_finetune_sgd_with_rules_against_a_torch_loop_with_param_groups(gpu_device):
    """Three steps against torch.optim.SGD with one real param_group per set of values, the backward started from the kernel's
    dlogits: the bars of tests/test_gpu_finetune.py::test_engine_against_torch_adam_loop — every loss to rtol 1e-4, the
    classifier everywhere and at least 95 % of all elements within rtol 1e-4 / atol 1e-6.  Those bars are absolute (atol 1e-6)
    and were set for a loop at lr 1e-4, where three steps move an element by a few 1e-4 at the most and two trajectories that
    differ in the last ulp of an update (torch's foreach SGD fuses its multiply-adds) drift apart by lr times the difference of
    their gradients; the loop here runs at that lr.  (At the lr 1e-3 of the other engine tests the same three steps leave 10 of
    the classifier's 51 712 weights outside, by at most 2.1e-6, and 1.8 % of all elements — the drift scales with lr, the
    bars do not.)"""
    import copy
    import test_gpu_finetune as FT
    from avid_hip import parallel
    dev, lr = gpu_device, 1e-4
    vids, labs = _finetune_inputs(dev, 3)
    m0 = FT._wrapper(dev)
    m_eng, m_ref = copy.deepcopy(m0), copy.deepcopy(m0)
    eng = parallel.FinetuneStep(m_eng, lr=lr, optimizer="sgd", momentum=0.9, nesterov=True, weight_decay=1e-4,
                                param_rules=_tower_rules(m_eng))
    vals = {n: (s, w) for n, s, w, _ in eng.param_values()}
    groups = {}
    for n, p in m_ref.named_parameters():
        groups.setdefault(vals[n], []).append(p)
    assert len(groups) == 4
    opt = torch.optim.SGD([{"params": ps, "lr": lr * s, "weight_decay": w} for (s, w), ps in groups.items()], lr=lr, momentum=0.9,
                          nesterov=True)
    le, lt = [], []
    for i in range(3):
        loss, _ = eng.step(vids[i], labs[i])
        le.append(float(loss))
        lt.append(FT._plain_step(m_ref, opt, vids[i], labs[i], True))
    torch.cuda.synchronize()
    np.testing.assert_allclose(le, lt, rtol=1e-4)
    off = FT._off_bar(m_eng, m_ref)
    total = sum(p.numel() for p in m_eng.parameters())
    print(f"\n[finetune sgd + rules] losses {le} against torch {lt}; outside the bars: {sum(k for k, _, _ in off.values())} of {total}")
    assert not any(n.startswith("classifier.") for n in off), off
    assert sum(k for k, _, _ in off.values()) <= 0.05 * total, off


def _engine(kind, dev, optimizer, **kw):
    """(engine, step(i)) of one of the three engines under ``optimizer`` at the sizes of tests/test_gpu_sgd.py's engine tests."""
    from avid_hip import parallel
    opt = dict(optimizer=optimizer, lr=1e-3, weight_decay=1e-4)
    opt.update(dict(momentum=0.9, nesterov=True) if optimizer in ("sgd", "lars") else {})
    opt.update(kw)
    if kind == "train":
        import test_gpu_engine as E
        import test_gpu_sgd as S
        video, audio, ids = E._data(dev, steps=4)
        m, crit, eng = S._trainstep(dev, **opt)
        return eng, m, lambda i: eng.step(video, audio, ids[i])
    if kind == "finetune":
        import test_gpu_finetune as FT
        vids, labs = _finetune_inputs(dev, 4)
        m = FT._wrapper(dev)
        eng = parallel.FinetuneStep(m, **opt)
        return eng, m, lambda i: eng.step(vids[i], labs[i])
    import test_gpu_probe as PR
    vids, labs = _probe_inputs(dev, 4)
    m = PR._model(dev)
    eng = parallel.ProbeStep(m, **opt)
    return eng, m, lambda i: eng.step(vids[i], labs[i])


@pytest.mark.parametrize("optimizer", ["lars", "lamb"])
@pytest.mark.parametrize("kind", ["train", "finetune", "probe"])
def test_engine_step_is_the_op_on_its_own_gradient(gpu_device, kind, optimizer):
    """Two steps: parameters, optimizer state, device step counter and trust array are what the op-level call gives on clones of
    the buffers from before the step and the gradient the step left — bit for bit."""
    eng, m, step = _engine(kind, gpu_device, optimizer, param_rules=None)
    assert eng._table_on and eng.trust is not None
    for i in range(2):
        snap = _snapshot(eng)
        step(i)
        torch.cuda.synchronize()
        tab = _op_on_snapshot(eng, snap)
        _assert_engine_is(eng, snap, tab)
    assert eng.t == 2
    sd = eng.state_dict()
    assert ("momentum" if optimizer == "lars" else "betas") in sd["param_groups"][0]           # torch.optim.SGD's / Adam's format
    assert len(sd["avid_param_table"]) == len(eng.flat.params)
    if kind == "train":
        assert eng._step_plan is not None, "the step did not run through a launch program"


def test_virtual_ranks_go_through_grad_scale(gpu_device):
    import test_gpu_finetune as FT
    from avid_hip import parallel
    dev = gpu_device
    vids, labs = _finetune_inputs(dev, 1, batch=8)
    m = FT._wrapper(dev)
    eng = parallel.FinetuneStep(m, lr=1e-3, optimizer="lars", momentum=0.9, weight_decay=1e-4, virtual_ranks=2,
                                param_rules=parallel.rules_no_decay_1d(m))
    snap = _snapshot(eng)
    eng.step(vids[0], labs[0])
    torch.cuda.synchronize()
    tab = _op_on_snapshot(eng, snap, grad_scale=0.5)          # the buffer holds the two replicas' SUM
    _assert_engine_is(eng, snap, tab)
    assert all(q == 1.0 for q, a in zip(eng.trust.tolist(), tab.adapt) if not a) and not all(tab.adapt)


@pytest.mark.parametrize("optimizer", ["lars", "lamb"])
def test_skipped_step_leaves_no_trace(gpu_device, optimizer):
    eng, m, step = _engine("probe", gpu_device, optimizer, skip_nonfinite=True)
    step(0)
    torch.cuda.synchronize()
    before, trust = _snapshot(eng), eng.trust.clone()
    assert not bool((trust == 1.0).all()) and int(eng.guard.skipped_total) == 0
    import test_gpu_probe as PR      # noqa: F401
    vids, labs = _probe_inputs(gpu_device, 1, seed=10)
    vids[0][0, 0, 0, 0, 0] = float("nan")
    eng.step(vids[0], labs[0])
    torch.cuda.synchronize()
    assert int(eng.guard.skipped) == 1 and int(eng.guard.skipped_total) == 1
    _assert_engine_is(eng, before)
    assert _same_bits(eng.trust, trust)
    step(1)
    torch.cuda.synchronize()
    assert int(eng.guard.skipped) == 0 and not _same_bits(eng.flat.flat, before["p"])


def test_average_and_set_lr_under_lars(gpu_device):
    """``ema_decay``: the average is the restatement of the parameters the step left, ``with ema_weights():`` puts it into the model.
    ``set_lr(0)`` reaches the next step: the momentum buffer moves, the parameters do not."""
    eng, m, step = _engine("probe", gpu_device, "lars", ema_decay=0.9)
    e0 = eng.ema.clone()
    step(0)
    torch.cuda.synchronize()
    assert _same_bits(eng.ema, ema_update(e0.cpu().numpy(), eng.flat.flat.cpu().numpy(), 0.9)) and int(eng.ema_updates) == 1
    live, avg = eng.flat.flat.clone(), eng.ema.clone()
    with eng.ema_weights():
        assert _same_bits(eng.flat.flat, avg) and not _same_bits(eng.flat.flat, live)
        assert all(_same_bits(p, eng.flat.view(avg, i)) for i, p in enumerate(eng.flat.params))
    assert _same_bits(eng.flat.flat, live)
    eng.set_lr(0.0)
    buf = eng.momentum_buffer.clone()
    step(1)
    torch.cuda.synchronize()
    assert _same_bits(eng.flat.flat, live) and not _same_bits(eng.momentum_buffer, buf)
    eng.set_lr(1e-3)
    step(2)
    torch.cuda.synchronize()
    assert not _same_bits(eng.flat.flat, live)


@pytest.mark.parametrize("optimizer", ["lars", "lamb"])
def test_checkpoint_resumes_with_the_same_bits(gpu_device, optimizer):
    import test_gpu_probe as PR
    from avid_hip import parallel
    dev = gpu_device
    eng, m, step = _engine("probe", dev, optimizer, param_rules=None)
    for i in range(2):
        step(i)
    torch.cuda.synchronize()
    sd = eng.state_dict()
    assert "avid_param_table" in sd
    m2 = PR._model(dev, seed=1)
    m2.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    kw = dict(momentum=0.5) if optimizer == "lars" else {}
    eng2 = parallel.ProbeStep(m2, lr=1.0, weight_decay=1e-4, optimizer=optimizer, **kw)
    eng2.load_state_dict(sd)
    vids, labs = _probe_inputs(dev, 4)
    step(2)
    eng2.step(vids[2], labs[2])
    torch.cuda.synchronize()
    assert _same_bits(eng2.flat.flat, eng.flat.flat) and _same_bits(eng2.trust, eng.trust)
    for name in ("momentum_buffer", "m", "v"):
        if getattr(eng, name) is not None:
            assert _same_bits(getattr(eng2, name), getattr(eng, name)), name
    with pytest.raises(ValueError, match="avid_param_table"):
        m3 = PR._model(dev, seed=2)
        parallel.ProbeStep(m3, lr=1.0, weight_decay=1e-4, optimizer=optimizer, param_rules=parallel.rules_no_decay_1d(m3),
                           **kw).load_state_dict(sd)


def test_captured_lamb_step_replays_as_the_eager_one(gpu_device):
    """Set up as tests/test_gpu_sgd.py::test_learning_rate_reaches_a_captured_sgd_graph: two eager steps, a capture, replays
    against an eager twin — the two passes, the finish and the trust array live in the graph, nothing reads the host."""
    import test_gpu_engine as E
    import test_gpu_sgd as S
    dev = gpu_device
    video, audio, ids = E._data(dev)
    kw = dict(lr=1e-3, optimizer="lamb", weight_decay=1e-4)
    m, c, e = S._trainstep(dev, **kw)
    m2, c2, twin = S._trainstep(dev, **kw)
    for i in range(2):
        e.step(video, audio, ids[i])
        twin.step(video, audio, ids[i])
    e.capture(video, audio, ids[2])
    torch.cuda.synchronize()
    assert e.t == 2 and int(e.t_dev) == 2
    assert _same_bits(e.flat.flat, twin.flat.flat)
    for lr, i in ((1e-3, 2), (0.0, 3), (3e-3, 4)):
        e.set_lr(lr)
        twin.set_lr(lr)
        before = e.flat.flat.clone()
        e.replay(index=ids[i])
        twin.step(video, audio, ids[i])
        torch.cuda.synchronize()
        assert _same_bits(e.flat.flat, before) == (lr == 0.0), lr
        assert _same_bits(e.flat.flat, twin.flat.flat) and _same_bits(e.m, twin.m) and _same_bits(e.v, twin.v), lr
        assert _same_bits(e.trust, twin.trust)
    assert e.t == 5 and int(e.t_dev) == 5


def test_default_engines_launch_none_of_the_new_kernels(gpu_device, kernel_log):
    """Without rules ``"adam"`` and ``"sgd"`` run exactly what they ran: the launch log of a step names ``adam_flat_kernel`` /
    ``sgd_flat_kernel`` and none of the table-driven kernels.  (Passes without the feature too.)"""
    new = ("seg_", "sgd_table", "sgd_flat_table", "adam_flat_table", "lamb_")
    for optimizer, old in (("adam", "adam_flat_kernel"), ("sgd", "sgd_flat_kernel")):
        eng, m, step = _engine("probe", gpu_device, optimizer)
        step(0)
        with kernel_log() as log:
            step(1)
        assert log.launches(old) == 1, sorted(log.report)
        assert not [k for k in log.report if k.startswith(new)], sorted(log.report)
    import test_gpu_engine as E
    video, audio, ids = E._data(gpu_device)
    m, crit, eng = E._make(gpu_device)
    eng.step(video, audio, ids[0])
    with kernel_log() as log:
        eng.step(video, audio, ids[1])
    assert log.launches("adam_flat_kernel") >= 1 and not [k for k in log.report if k.startswith(new)], sorted(log.report)
