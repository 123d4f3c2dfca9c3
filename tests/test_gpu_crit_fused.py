"""``ops.crit_fused`` (``avid_crit_fused``: any AVID / AVID+CMA term set in one kernel, Z frozen) on the GPU against its float64
restatement (tests/_crit_ref.py, pinned on the CPU by tests/test_crit_fused_host.py), against the stock entry points at the two
stock term sets, through the criterions against the unfused chain, and under guard bands.

Bars (those of the stock fused kernels, tests/test_gpu_ops.py): losses rtol 2e-6, normalised embeddings 1e-6, gradients 2e-5 of
their scale with an upstream gradient of 2.0, repeated calls bit-identical, the device error word clean.

Shapes: the smallest that cross every edge of a 64-row block (1 + P + K = 64 and 65, a one-row last block, K < 64) and of the
K-vs-Kw split (Kw = K, Kw = 1, Kw inside the first block, Kw = 64 of 1024), and one full-size case."""
import functools

import numpy as np
import pytest
import torch

import _crit_ref as R
from _guards import FILLS, guarded

pytestmark = pytest.mark.gpu

CMA_SHAPES = [(3, 5, 70, 70, 300), (4, 1, 33, 7, 200), (2, 3, 60, 1, 200), (2, 3, 61, 61, 200), (6, 32, 1024, 64, 5000)]   # bs, P, K, Kw, N
AVID_SHAPES = [(3, 0, K, K, 300) for K in (63, 64, 65, 129)]


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@functools.lru_cache(maxsize=None)
def case(mask, shape, coeffs=R.COEFFS):
    """The float64 figures of one (term set, shape): computed once, shared, never modified."""
    return R.crit_case(mask, *shape, coeffs=coeffs)


def run(c, dev, mask, coeffs, Kw, repeats=1, idx=None, P=lambda t: t):
    """``ops.crit_fused`` on the inputs of ``c``: ([(total, losses, hats)] * repeats, the leaf embeddings, the workspace)."""
    from avid_hip import ops
    bs, K, Pn = c.ve.shape[0], c.idx.shape[1], 0 if c.pos is None else c.pos.shape[1]
    vd, ad = P(c.ve.to(dev).requires_grad_(True)), P(c.ae.to(dev).requires_grad_(True))
    ws = ops.crit_fused_workspace(dev, bs, Pn, K)
    args = (P(c.y.to(dev)), None if c.pos is None else P(c.pos.to(dev)), P((c.idx if idx is None else idx).to(dev)),
            P(c.v1.to(dev)), P(c.v2.to(dev)), P(c.Z.to(dev)), 1 / c.T, Kw, mask, coeffs, ws)
    return [ops.crit_fused(vd, ad, *args) for _ in range(repeats)], vd, ad, ws


def check(c, outs, vd, ad, what):
    total, losses, hats = outs[0]
    assert all(torch.equal(o[0], total) and torch.equal(o[1], losses) and torch.equal(o[2], hats) for o in outs[1:]), what
    (total * 2.0).backward()
    got = losses.cpu().numpy()
    print(what, "losses", np.abs(got[:13] - c.losses).max() / max(abs(x) for x in c.losses), "hats", relerr(hats[0], c.vh),
          relerr(hats[1], c.ah), "grads", relerr(vd.grad, 2.0 * c.gv), relerr(ad.grad, 2.0 * c.ga))
    np.testing.assert_allclose(got[:13], c.losses, rtol=2e-6, atol=0, err_msg=what)
    off = [k for k in range(8) if not c.mask >> (k // 2) & 1]
    assert all(got[k] == 0.0 for k in off + [8 + k // 2 for k in off] + [13, 14, 15]), (what, got)
    assert float(total.detach()) == float(got[12])
    assert relerr(hats[0], c.vh) < 1e-6 and relerr(hats[1], c.ah) < 1e-6, what
    assert relerr(vd.grad, 2.0 * c.gv) < 2e-5 and relerr(ad.grad, 2.0 * c.ga) < 2e-5, what
    return got


@pytest.mark.parametrize("shape", AVID_SHAPES + CMA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_term_sets_vs_fp64(shape, gpu_device):
    """Every mask the criterions can produce, the two stock ones included, at every shape; the inputs carry an id equal to N - 1
    in y and in idx and (from bs = 3 on) a duplicate id in y."""
    from avid_hip import ops
    bs, P, K, Kw, N = shape
    masks = (R.X_INST,) + R.AVID_MASKS if P == 0 else R.CMA_MASKS + (R.X_INST | R.W_POS,)
    ops.check_device_errors(gpu_device)
    for mask in masks:
        c = case(mask, shape)
        assert int(c.y[0]) == N - 1 and int(c.idx[-1, -1]) == N - 1 and (bs < 3 or int(c.y[2]) == int(c.y[1]))
        outs, vd, ad, _ = run(c, gpu_device, mask, R.COEFFS, Kw, repeats=3)
        check(c, outs, vd, ad, f"mask {mask} shape {shape}")
    ops.check_device_errors(gpu_device)


@pytest.mark.parametrize("shape", [AVID_SHAPES[2], CMA_SHAPES[1], CMA_SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_stock_masks_agree_with_the_stock_entry_points(shape, gpu_device):
    """X_INST at P = 0 against ops.xmodal_fused, X_INST | W_POS against ops.cma_fused: the same inputs, the same bars (the two
    kernels differ in how they place the sample's own row and the loss terms' partial sums: no bit-identity is asked)."""
    from avid_hip import ops
    bs, P, K, Kw, N = shape
    dev = gpu_device
    mask = R.X_INST if P == 0 else R.X_INST | R.W_POS
    c = case(mask, shape)
    (new,), vd, ad, _ = run(c, dev, mask, R.COEFFS, Kw)
    (new[0] * 2.0).backward()
    vo, ao = c.ve.to(dev).requires_grad_(True), c.ae.to(dev).requires_grad_(True)
    if P == 0:
        total, losses, hats = ops.xmodal_fused(vo, ao, c.y.to(dev), c.idx.to(dev), c.v1.to(dev), c.v2.to(dev), c.Z.to(dev), 1 / c.T,
                                               R.COEFFS[0], ops.xmodal_fused_workspace(dev, bs, K))
        pairs = ((0, 0), (1, 1), (8, 2), (12, 3))                          # (index in losses[16], index in the stock losses)
    else:
        total, losses, hats = ops.cma_fused(vo, ao, c.y.to(dev), c.pos.to(dev), c.idx.to(dev), c.v1.to(dev), c.v2.to(dev),
                                            c.Z.to(dev), 1 / c.T, Kw, R.COEFFS[0], R.COEFFS[3],
                                            ops.cma_fused_workspace(dev, bs, P, K))
        pairs = ((0, 0), (1, 1), (6, 2), (7, 3), (8, 4), (11, 5), (12, 6))
    (total * 2.0).backward()
    n, o = new[1].cpu().numpy(), losses.cpu().numpy()
    np.testing.assert_allclose([n[i] for i, _ in pairs], [o[j] for _, j in pairs], rtol=2e-6, atol=0)
    assert relerr(new[2], hats) < 1e-6
    assert relerr(vd.grad, vo.grad) < 2e-5 and relerr(ad.grad, ao.grad) < 2e-5
    ops.check_device_errors(dev)


def test_zero_coefficient_reports_the_loss_and_carries_no_gradient(gpu_device):
    """A set bit with coefficient 0 (AVID+CMA with wModalInst alone puts X_INST there): its two losses are the term's, the
    gradient is the gradient of the other terms alone."""
    shape, mask, coeffs = CMA_SHAPES[1], R.X_INST | R.X_POS | R.W_POS, (0.4, 0., 0., 0.3)
    c = case(mask, shape, coeffs)
    outs, vd, ad, _ = run(c, gpu_device, mask, coeffs, shape[3], repeats=2)
    got = check(c, outs, vd, ad, "X_POS at coefficient 0")
    assert got[4] > 0 and got[5] > 0 and got[10] > 0
    without = case(R.X_INST | R.W_POS, shape, coeffs)                      # float64, the term off altogether
    np.testing.assert_allclose(got[12], without.losses[12], rtol=2e-6)
    assert relerr(vd.grad, 2.0 * without.gv) < 2e-5 and relerr(ad.grad, 2.0 * without.ga) < 2e-5
    lone = case(R.X_INST, shape, (0., 0., 0., 0.))                         # every coefficient 0: losses, a zero gradient
    outs, vd, ad, _ = run(lone, gpu_device, R.X_INST, (0., 0., 0., 0.), shape[3])
    (outs[0][0] * 2.0).backward()
    np.testing.assert_allclose(outs[0][1].cpu().numpy()[:2], lone.losses[:2], rtol=2e-6)
    assert float(outs[0][0].detach()) == 0.0 and not vd.grad.any() and not ad.grad.any()


def test_out_of_range_id_sets_the_error_word_and_stays_inside_the_bank(gpu_device):
    """The reference raises on such an id (criterions/avid.py:57-62); the kernel flags it, reads the nearest row of the bank
    instead and leaves finite outputs — those of the clamped ids."""
    from avid_hip import ops
    shape, mask = CMA_SHAPES[1], R.X_INST | R.X_POS | R.W_POS
    bs, P, K, Kw, N = shape
    c = case(mask, shape)
    idx = c.idx.clone()
    idx[1, 3], idx[2, K - 1] = N + 5, -3
    ops.check_device_errors(gpu_device)
    outs, vd, ad, _ = run(c, gpu_device, mask, R.COEFFS, Kw, idx=idx)
    total, losses, hats = outs[0]
    total.backward()
    with pytest.raises(IndexError, match="outside"):
        ops.check_device_errors(gpu_device)
    assert all(bool(torch.isfinite(t).all()) for t in (losses, hats, vd.grad, ad.grad))
    ref = R.crit_ref(c.ve, c.ae, c.v1, c.v2, c.y, c.pos, idx.clamp(0, N - 1), c.Z, mask, R.COEFFS, Kw)
    np.testing.assert_allclose(losses.cpu().numpy()[:13], ref.losses, rtol=2e-6, atol=0)
    ops.check_device_errors(gpu_device)                                    # the flag was cleared by the raise


# ------------------------------------------------------------------------------------------------ through the criterions
def _two_steps(make, gpu_device, monkeypatch):
    from avid_hip import ops
    res, calls = [], []
    real = ops.crit_fused
    monkeypatch.setattr(ops, "crit_fused", lambda *a: (calls.append(a[10]), real(*a))[1])
    for fused in (True, False):
        monkeypatch.setattr(ops, "FUSED_CRITERION", fused)
        torch.manual_seed(5)
        c = make()
        g = torch.Generator().manual_seed(11)
        out = []
        for step in range(2):
            v = torch.randn(6, 128, generator=g).to(gpu_device).requires_grad_(True)
            a = torch.randn(6, 128, generator=g).to(gpu_device).requires_grad_(True)
            yy = torch.randperm(3000, generator=g)[:6].to(gpu_device)
            n = len(calls)
            loss, tb = c(v, a, yy)
            loss.backward()
            assert len(calls) - n == (1 if fused and step == 1 else 0)     # step 2, and only it, went through ops.crit_fused
            out.append((float(loss), {k: float(x) for k, x in tb.items()}, v.grad.clone(), a.grad.clone()))
        res.append((out, c.nce_average.view1_mem.clone(), c.nce_average.view2_mem.clone()))
    ops.check_device_errors(gpu_device)
    (f, fb1, fb2), (u, ub1, ub2) = res
    assert f[0][0] == u[0][0]                                              # the first step is the unfused path either way
    np.testing.assert_allclose(f[1][0], u[1][0], rtol=3e-6)
    assert list(f[1][1]) == list(u[1][1])
    for k in f[1][1]:
        np.testing.assert_allclose(f[1][1][k], u[1][1][k], rtol=3e-6, err_msg=k)
    assert relerr(f[1][2], u[1][2]) < 2e-5 and relerr(f[1][3], u[1][3]) < 2e-5
    assert relerr(fb1, ub1) < 1e-6 and relerr(fb2, ub2) < 1e-6
    return calls


@pytest.mark.parametrize("xc,wc", [(1., 1.), (0., 1.)], ids=["joint", "self"])
def test_avid_criterion_fused_step_equals_the_unfused_one(xc, wc, gpu_device, monkeypatch):
    import criterions
    calls = _two_steps(lambda: criterions.AVID(num_data=3000, embedding_dim=128, num_negatives=256, momentum=0.5, xModal_coeff=xc,
                                               wModal_coeff=wc, device=gpu_device.index or 0), gpu_device, monkeypatch)
    assert calls == [(R.X_INST if xc else 0) | R.W_INST]


def test_avid_cma_all_groups_fused_step_equals_the_unfused_one(gpu_device, monkeypatch):
    import criterions
    calls = _two_steps(lambda: criterions.AVID_CMA(num_data=3000, embedding_dim=128, num_negatives=256, num_negatives_within=32,
                                                   momentum=0.5, xModalInstCoeff=.25, wModalInstCoeff=.25, xModalPosCoeff=.25,
                                                   wModalPosCoeff=.25, sampling_args={"type": "consensus", "pos_k": 8},
                                                   device=gpu_device.index or 0), gpu_device, monkeypatch)
    assert calls == [R.X_INST | R.X_POS | R.W_POS]


# ------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("mask,shape", [(R.X_INST | R.W_INST, (3, 0, 70, 70, 300)), (R.X_INST | R.X_POS | R.W_POS, (4, 1, 33, 7, 200))],
                         ids=["avid-joint", "cma-all"])
def test_no_write_outside_and_no_read_of_unwritten_memory(mask, shape, gpu_device):
    """As tests/test_gpu_guards.py for ``cma_fused``: every allocation between guard bands and poisoned, the workspace exactly
    ``avid_crit_fused_workspace_bytes``; no guard byte changes, and all 16 losses and every other output are the same bits under
    both fills and in the plain run."""
    from avid_hip import lib, ops
    bs, P, K, Kw, N = shape
    c = case(mask, shape)

    def once(place):
        outs, vd, ad, ws = run(c, gpu_device, mask, R.COEFFS, Kw, repeats=2, P=place)      # the second call: the re-armed ticket
        (outs[1][0] * 2.0).backward()
        ops.check_device_errors(gpu_device)
        res = {"total0": outs[0][0], "total": outs[1][0], "losses": outs[1][1], "hats": outs[1][2], "dv": vd.grad, "da": ad.grad}
        return {k: v.detach().clone() for k, v in res.items()}, ws
    plain, _ = once(lambda t: t)
    assert plain["losses"].numel() == 16
    runs = []
    for fill in FILLS:
        with guarded(fill) as g:
            res, ws = once(g.place)
            torch.cuda.synchronize()
            g.check()
            need = int(lib.raw("avid_crit_fused_workspace_bytes")(bs, P, K))
            assert ws.numel() == need and need in g.size_values
            assert any(r.kind == "input" for r in g.records) and any(r.nbytes == need and r.kind == "zeros" for r in g.records)
        runs.append(res)
    for k in plain:
        assert torch.equal(runs[0][k], runs[1][k]), f"'{k}' depends on unwritten memory (0xFF vs 0x5A fill)"
        assert torch.equal(runs[0][k], plain[k]), f"'{k}' differs from the plain run"
