"""The criterion kernels at embedding widths other than 128, and the block edges of the fused and multi-block kernels.

``avid_bank_scores_*`` have four template instances (D = 64, 128, 256, 512), ``avid_l2norm_*`` and ``avid_bank_update*`` loop
over 64-wide trips with a ragged last one, ``avid_cma_topk`` / ``avid_knn_search`` take any multiple of 32 — and
``criterions.AVID(embedding_dim=...)`` puts all of them on the training path the moment a config asks for another width.  Here
every one of them runs against the float64 restatements of tests/_width_ref.py and is held to the per-element error bounds
derived there from each kernel's summation structure (c * u * sum |terms|, not a fraction of the output's scale);
tests/test_embedding_widths_host.py shows on the CPU that float32 arithmetic stays inside those bounds and that a dropped
64-float slice, a row pitch left at 128, a neighbouring or dropped row and the wrong duplicate each land >= 10 x outside them
at these very inputs.  Shapes: the smallest at which each path exists (tests/_width_ref.py).
"""
import numpy as np
import pytest
import torch

import _knn_ref as R
import _width_ref as W
from _fused_ref import cma_case, xmodal_case
from oracle import avid_oracle as O

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def within(what, got, want, bound):
    """Every element of ``got`` within ``bound`` of ``want`` (bound 0: equal); prints the largest fraction of the bound used."""
    diff = np.abs(got.detach().double().cpu().numpy() - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / bound)
    print(f"{what}: largest error {diff.max():.3e}, at most {r.max():.3f} of the bound")
    assert np.isfinite(diff).all() and (diff <= bound).all(), f"{what}: {int((diff > bound).sum())} elements outside the bound, worst {r.max():.3g} x"


# ---- a. F.normalize -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", W.L2_BS)
@pytest.mark.parametrize("D", W.L2_WIDTHS)
def test_l2_normalize_widths(D, bs, gpu_device):
    from avid_hip import ops
    x, dy = W.l2_inputs(bs, D)
    xd = x.to(gpu_device).requires_grad_(True)
    y = ops.l2_normalize(xd)
    y.backward(dy.to(gpu_device))
    within(f"l2 forward D {D} bs {bs}", y, W.normalize_fwd(x)[0], W.normalize_fwd_bound(x))
    keep = np.ones(bs, bool)
    if bs > W.L2_ZERO_ROW:
        assert bool((y[W.L2_ZERO_ROW] == 0).all())                 # the clamped zero row: exactly 0
        keep[W.L2_ZERO_ROW] = False                                # (its gradient is dy / 1e-12: the one masked row)
    within(f"l2 backward D {D} bs {bs}", xd.grad[torch.from_numpy(keep)], W.normalize_bwd(x, dy)[keep], W.normalize_bwd_bound(x, dy)[keep])


# ---- b. bank_scores -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,R", W.SCORE_SHAPES)
@pytest.mark.parametrize("D", W.SCORE_WIDTHS)
def test_bank_scores_widths(D, bs, R, gpu_device, kernel_log):
    from avid_hip import ops
    bank, emb, idx, ds = W.score_inputs(D, bs, R)
    ed = emb.to(gpu_device).requires_grad_(True)
    bank_d, idx_d = bank.to(gpu_device), idx.to(gpu_device)
    with kernel_log() as log:
        s = ops.bank_scores(ed, bank_d, idx_d, W.INV_T)
        s_plain = ops.bank_scores(ed.detach(), bank_d, idx_d, W.INV_T)        # no gradient wanted: no snapshot
        bank_d.zero_()                                                        # backward must read its snapshot, at pitch D
        s.backward(ds.to(gpu_device))
    assert log.launches("bank_scores_fwd_kernel") == 2 and log.launches("bank_scores_bwd_kernel") == 1
    assert s_plain.grad_fn is None and torch.equal(s.detach(), s_plain)
    within(f"scores D {D} bs {bs} R {R}", s, W.scores(bank, emb, idx), W.scores_bound(bank, emb, idx))
    within(f"d emb D {D} bs {bs} R {R}", ed.grad, W.scores_grad(bank, idx, ds), W.scores_grad_bound(bank, idx, ds))
    ops.check_device_errors(gpu_device)


# ---- c. the two forms of avid_bank_scores_bwd that the Python layer never calls ---------------------------------------------
@pytest.mark.parametrize("R", W.ABI_R)
@pytest.mark.parametrize("D", W.ABI_WIDTHS)
def test_bank_scores_bwd_regather_and_accumulate_forms(D, R, gpu_device):
    """include/avid_hip.h: ``rows == NULL`` re-gathers ``bank[idx]`` (the same rows in the same order as the snapshot: the same
    bits); ``accumulate = 1`` adds to ``demb``: the pre-fill plus the ``accumulate = 0`` result, one float32 addition each."""
    from avid_hip import lib, ops
    bs, N = 3, W.SCORE_N
    bank, emb, idx, ds = W.score_inputs(D, bs, R)
    bank_d, idx_d, ds_d = bank.to(gpu_device), idx.to(gpu_device), ds.to(gpu_device)
    rows = bank_d[idx_d].contiguous()                                         # the snapshot: [bs, R, D]
    p, st = ops._p, ops._stream()
    pre = (torch.rand(bs, D, generator=torch.Generator().manual_seed(D + R)) * 8 - 4).to(gpu_device)
    snap, gath = torch.empty(bs, D, device=gpu_device), torch.empty(bs, D, device=gpu_device)
    acc_s, acc_g = pre.clone(), pre.clone()
    lib.call("avid_bank_scores_bwd", bs, R, D, 0, p(rows), None, None, p(ds_d), W.INV_T, 0, p(snap), st)
    lib.call("avid_bank_scores_bwd", bs, R, D, N, None, p(idx_d), p(bank_d), p(ds_d), W.INV_T, 0, p(gath), st)
    lib.call("avid_bank_scores_bwd", bs, R, D, 0, p(rows), None, None, p(ds_d), W.INV_T, 1, p(acc_s), st)
    lib.call("avid_bank_scores_bwd", bs, R, D, N, None, p(idx_d), p(bank_d), p(ds_d), W.INV_T, 1, p(acc_g), st)
    within(f"snapshot form D {D} R {R}", snap, W.scores_grad(bank, idx, ds), W.scores_grad_bound(bank, idx, ds))
    assert torch.equal(gath, snap), "the re-gather form differs from the snapshot form"
    exact = pre.double().cpu().numpy() + snap.double().cpu().numpy()
    within(f"accumulate form D {D} R {R}", acc_s, exact, W.U * np.abs(exact))
    assert torch.equal(acc_g, acc_s)


# ---- d. bank_update / bank_update_pair ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", W.UPDATE_B)
@pytest.mark.parametrize("D", W.UPDATE_WIDTHS)
def test_bank_update_widths(D, B, gpu_device):
    from avid_hip import ops
    bank, emb0, emb1, y = W.update_inputs(D, B)
    m0, m1 = W.MOMENTA
    e0, e1, yd = emb0.to(gpu_device), emb1.to(gpu_device), y.to(gpu_device)
    b0, b1, p0, p1 = (bank.to(gpu_device) for _ in range(4))
    ops.bank_update(b0, yd, e0, m0)
    ops.bank_update(b1, yd, e1, m1)
    ops.bank_update_pair(p0, p1, yd, e0, e1, m0, m1)
    ops.check_device_errors(gpu_device)
    assert torch.equal(p0, b0) and torch.equal(p1, b1)             # one launch == two launches, bit for bit
    owned = torch.unique(y)
    untouched = np.setdiff1d(np.arange(W.UPDATE_N), y.numpy())
    for got, emb, m in ((b0, emb0, m0), (b1, emb1, m1)):
        want, bound = W.bank_update(bank, y, emb, m)
        within(f"update D {D} B {B} m {m}", got, want, bound)      # (bound 0 off the owned rows: their bits are kept)
        assert torch.equal(got.cpu()[untouched], bank[untouched])
        np.testing.assert_allclose(got.cpu()[owned].double().norm(dim=1).numpy(), 1.0, rtol=1e-6)


@pytest.mark.parametrize("bad", [-1, W.UPDATE_N], ids=["id=-1", "id=N"])
@pytest.mark.parametrize("D", [100, 512])
def test_bank_update_flags_an_id_outside_the_bank(D, bad, gpu_device):
    """index_copy_ would raise (criterions/avid.py:124): the kernels flag the id and write nothing."""
    from avid_hip import ops
    bank, emb0, emb1, _ = W.update_inputs(D, 1)
    yd = torch.tensor([bad], device=gpu_device)
    b0, p0, p1 = (bank.to(gpu_device) for _ in range(3))
    ops.check_device_errors(gpu_device)
    ops.bank_update(b0, yd, emb0.to(gpu_device), 0.5)
    with pytest.raises(IndexError, match="update_memory"):
        ops.check_device_errors(gpu_device)
    ops.bank_update_pair(p0, p1, yd, emb0.to(gpu_device), emb1.to(gpu_device), 0.5, 0.9)
    with pytest.raises(IndexError, match="update_memory"):
        ops.check_device_errors(gpu_device)
    assert all(torch.equal(t.cpu(), bank) for t in (b0, p0, p1))
    ops.check_device_errors(gpu_device)                                       # the flag was cleared


def test_bank_update_refuses_a_width_above_512(gpu_device, kernel_log):
    from avid_hip import ops
    from avid_hip.lib import AvidHipError
    g = torch.Generator().manual_seed(513)
    bank, emb = torch.randn(20, 513, generator=g), torch.randn(2, 513, generator=g)
    b0, b1, e, yd = bank.to(gpu_device), bank.to(gpu_device), emb.to(gpu_device), torch.tensor([3, 7], device=gpu_device)
    with kernel_log() as log:
        with pytest.raises(AvidHipError, match="bank_update"):
            ops.bank_update(b0, yd, e, 0.5)
        with pytest.raises(AvidHipError, match="D=513"):
            ops.bank_update_pair(b0, b1, yd, e, e, 0.5, 0.9)
    assert not log.report and torch.equal(b0.cpu(), bank) and torch.equal(b1.cpu(), bank)


# ---- e. the argument checks of ops.bank_scores / bank_update / bank_update_pair ---------------------------------------------
def _refused(gpu_device, kernel_log, match, fn, tensors):
    """``fn()`` raises AvidHipError before anything is launched; every tensor keeps its bits."""
    from avid_hip.lib import AvidHipError
    before = [t.clone() for t in tensors]
    with kernel_log() as log:
        with pytest.raises(AvidHipError, match=match):
            fn()
    assert not log.report, f"launched: {sorted(log.report)}"
    assert all(torch.equal(a, b) for a, b in zip(tensors, before))


def test_bank_scores_refuses_mismatched_arguments(gpu_device, kernel_log):
    from avid_hip import ops
    bank, emb, idx, _ = (t.to(gpu_device) for t in W.score_inputs(128, 3, 17))
    wide = W.score_inputs(256, 3, 17)[1].to(gpu_device)
    for needs_grad in (False, True):
        e, w = emb.clone().requires_grad_(needs_grad), wide.clone().requires_grad_(needs_grad)
        _refused(gpu_device, kernel_log, "width 256 != bank width 128", lambda: ops.bank_scores(w, bank, idx, W.INV_T), [w, bank, idx])
        _refused(gpu_device, kernel_log, "width 128 != bank width 256", lambda: ops.bank_scores(e, W.score_inputs(256, 3, 17)[0].to(gpu_device), idx, W.INV_T), [e, idx])
        _refused(gpu_device, kernel_log, "float32", lambda: ops.bank_scores(e, bank.double(), idx, W.INV_T), [e, bank, idx])
        _refused(gpu_device, kernel_log, "idx has 2 rows, emb 3", lambda: ops.bank_scores(e, bank, idx[:2].contiguous(), W.INV_T), [e, bank, idx])
        _refused(gpu_device, kernel_log, "idx has 3 rows, emb 2", lambda: ops.bank_scores(e[:2], bank, idx, W.INV_T), [e, bank, idx])
        _refused(gpu_device, kernel_log, "int64", lambda: ops.bank_scores(e, bank, idx.int(), W.INV_T), [e, bank, idx])
    ops.check_device_errors(gpu_device)


def test_bank_update_refuses_mismatched_arguments(gpu_device, kernel_log):
    from avid_hip import ops
    bank, emb0, emb1, y = (t.to(gpu_device) for t in W.update_inputs(256, 5))
    narrow = W.update_inputs(100, 5)[1].to(gpu_device)
    other = W.update_inputs(100, 5)[0].to(gpu_device)                          # a bank of another width
    b0, b1 = bank.clone(), bank.clone()
    keep = [b0, b1, other, emb0, emb1, narrow, y]
    for match, args in (("width 100 != bank width 256", (b0, y, narrow)), ("width 256 != bank width 100", (other, y, emb0)),
                        ("y must be int64", (b0, y.int(), emb0)), ("y has 4 ids, emb 5 rows", (b0, y[:4], emb0)),
                        ("y has 5 ids, emb 4 rows", (b0, y, emb0[:4])), ("float32", (b0.double(), y, emb0))):
        _refused(gpu_device, kernel_log, "bank_update: .*" + match, lambda: ops.bank_update(*args, 0.5), keep)
    for match, args in (("width 100 != bank width 256", (b0, b1, y, emb0, narrow)), ("width 100 != bank width 256", (b0, b1, y, narrow, emb1)),
                        ("y must be int64", (b0, b1, y.int(), emb0, emb1)), ("y has 4 ids, emb 5 rows", (b0, b1, y[:4], emb0, emb1)),
                        ("y has 5 ids, emb 4 rows", (b0, b1, y, emb0, emb1[:4])), ("banks differ in shape", (b0, other, y, emb0, narrow)),
                        ("banks differ in shape", (b0, b1[:50], y, emb0, emb1))):
        _refused(gpu_device, kernel_log, "bank_update_pair: .*" + match, lambda: ops.bank_update_pair(*args, 0.5, 0.9), keep)
    assert torch.equal(b0, bank) and torch.equal(b1, bank)
    ops.check_device_errors(gpu_device)


# ---- f. the correspondence search and the k-NN search -----------------------------------------------------------------------
@pytest.mark.parametrize("N", W.TOPK_N)
@pytest.mark.parametrize("D", W.TOPK_WIDTHS)
def test_cma_topk_widths(D, N, gpu_device):
    """All four agreement kinds against the oracle's dense search by the rule of test_cma_topk_filter_path_vs_oracle (equal sets
    for > 99.8 % of the queries, >= k - 1 common rows for every one, rows ascending, never the query itself) and, for EVERY
    query, against the float64 scores: whatever scores above the k-th best by more than the float32 tolerance is present,
    nothing present scores below it by more (W.topk_check; the host test shows the oracle's float32 search passing it)."""
    from avid_hip import topk
    v1, v2 = W.topk_banks(N, D)
    d1, d2 = v1.to(gpu_device), v2.to(gpu_device)
    k = W.TOPK_K
    got = {}
    for kind, name in enumerate(W.TOPK_KINDS):
        got[name] = topk.cma_topk(d1, d2, 0, N, k, kind, batch=1024).cpu().numpy()
        want = O.cma_topk(v1, v2, k, name)
        assert got[name].shape == want.shape
        same = np.mean([set(got[name][i]) == set(want[i]) for i in range(N)])
        print(f"N {N} D {D} {name}: {same:.4%} of the sets equal the oracle's")
        assert same > 0.998, (name, same)
        for i in range(N):
            assert i not in set(got[name][i]) and len(set(got[name][i]) & set(want[i])) >= k - 1
        assert (np.diff(got[name], axis=1) > 0).all()
    for name, (same, common) in W.topk_check(N, D, got).items():
        print(f"N {N} D {D} {name}: {same:.4%} of the sets equal the float64 top-{k}, >= {common} rows in common")
        assert same > 0.998 and common >= k - 1
    a = topk.cma_topk(d1, d2, 0, N // 2 - 7, k, 0, batch=256)                  # sharded ranges, a ragged last batch
    b = topk.cma_topk(d1, d2, N // 2 - 7, N, k, 0, batch=128)
    assert torch.equal(torch.cat([a, b]).cpu(), torch.from_numpy(got["consensus"]))


@pytest.mark.parametrize("N", W.TOPK_N)
@pytest.mark.parametrize("D", W.TOPK_WIDTHS)
def test_knn_search_widths(D, N, gpu_device):
    """The rule of test_gpu_knn.test_search_on_random_unit_vectors (D = 128, 512) at D = 64, 256, for the exact scan (N = 500)
    and the threshold filter (N = 4608): against tests/_knn_ref.py in float64."""
    from avid_hip import ops
    k, Q, tol = 20, 130, W.topk_tolerance(D)
    gallery, queries = W.topk_banks(N, D)[0], W.topk_banks(N, D)[1][:Q].contiguous()
    want_i, want_s = R.search(gallery.numpy(), queries.numpy(), k)
    s64 = queries.double().numpy() @ gallery.double().numpy().T
    idx, sim = (t.cpu().numpy() for t in ops.knn_search(gallery.to(gpu_device), queries.to(gpu_device), k))
    assert idx.shape == (Q, k) and idx.min() >= 0 and idx.max() < N and all(len(set(r)) == k for r in idx)
    assert (np.diff(sim, axis=1) <= 0).all()
    pair = np.take_along_axis(s64, idx.astype(np.int64), 1)
    err = np.abs(sim - pair).max()
    print(f"N {N} D {D}: largest |sim - float64 dot| {err:.3e} (tolerance {tol:.3e}); {np.mean(idx == want_i):.4%} of the ranks equal")
    assert err <= tol
    kth = want_s[:, k - 1]
    must = s64 > (kth + 2 * tol)[:, None]
    present = np.zeros_like(must)
    np.put_along_axis(present, idx.astype(np.int64), True, 1)
    assert not (must & ~present).any()
    assert (pair >= (kth - 2 * tol)[:, None]).all()


# ---- g. criterions.AVID / AVID_CMA end to end -------------------------------------------------------------------------------
def _close(what, got, want, tol):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    print(f"{what}: {W.deviation(got, want, tol):.3f} of the tolerance (rtol {tol[0]:g}, atol {tol[1]:g})")
    np.testing.assert_allclose(got, want, rtol=tol[0], atol=tol[1], err_msg=what)


def _criterion(kind, D, dev):
    import criterions
    from criterions.avid_cma import AVIDSimilarityPositiveExpansion
    from criterions.nce import NCECriterion
    c = W.CRIT[kind]
    if kind == "avid":
        return criterions.AVID(num_data=c["N"], embedding_dim=D, num_negatives=c["K"], momentum=0.5, xModal_coeff=1.0,
                               wModal_coeff=1.0, device=dev.index)
    crit = criterions.AVID_CMA.__new__(criterions.AVID_CMA)       # (as the golden tests: the positive set is injected below)
    torch.nn.Module.__init__(crit)
    crit.nce_average = AVIDSimilarityPositiveExpansion(
        memory_size=c["N"], embedding_dim=D, num_negatives=c["K"], num_negatives_within=c["Kw"], xModalInst=True, wModalInst=True,
        xModalPos=True, wModalPos=True, sampling_args={"type": "consensus", "pos_k": c["pos_k"]}, momentum=0.5, device=dev.index)
    crit.xModalInstCoeff = crit.wModalInstCoeff = crit.xModalPosCoeff = crit.wModalPosCoeff = 0.25
    crit.criterion = NCECriterion(c["N"]).to(dev)
    return crit


@pytest.mark.parametrize("kind", ["avid", "cma"])
@pytest.mark.parametrize("D", W.CRIT_WIDTHS)
def test_criterion_two_steps(D, kind, gpu_device, kernel_log):
    """criterions.AVID (cross- and within-modal terms) and criterions.AVID_CMA (all four groups) at embedding_dim 64 and 256: two
    steps with injected negatives (AVID_CMA: injected ``rand_idx`` and the positive set of ``O.cma_topk`` of the test's banks)
    against ``O.avid_forward`` / ``O.avid_cma_forward`` in float64 — loss, every tb_log entry, Z after step 1 and carried into
    step 2, both embedding gradients, the updated rows of both banks — at the tolerances of
    test_avid_two_steps_vs_reference_golden (loss, Z, tb_log 5e-6; gradients rtol 2e-4 atol 2e-7; bank rows rtol 2e-6 atol 2e-7).

    Those were set against a float32 reference; what the float32 oracle itself uses of them against the float64 oracle, measured
    on the CPU by test_embedding_widths_host.test_float32_oracle_deviation_is_a_quarter_of_the_tolerances (largest of the two
    steps; all <= 1/4, so the tolerances stay as they are):

        kind  D    loss   Z      tb_log  gradients  bank rows
        avid  64   0.013  0.031  0.016   0.036      0.052
        avid  256  0.003  0.013  0.016   0.013      0.053
        cma   64   0.018  0.003  0.017   0.048      0.066
        cma   256  0.006  0.017  0.014   0.007      0.061

    Neither step may take a fused kernel (D != 128), and the unfused ``bank_scores_fwd_kernel`` must have run."""
    v1, v2, steps = W.crit_inputs(kind, D)
    want = W.oracle_steps(kind, D, torch.float64)
    crit = _criterion(kind, D, gpu_device)
    na = crit.nce_average
    na.view1_mem.copy_(v1)
    na.view2_mem.copy_(v2)
    if kind == "cma":
        na.register_buffer("positive_set", torch.from_numpy(W.positive_set(D)).to(gpu_device))
    z1 = None
    for step, ((v, a, y, draw), w) in enumerate(zip(steps, want)):
        vd, ad = v.to(gpu_device).requires_grad_(True), a.to(gpu_device).requires_grad_(True)
        yd, dd = y.to(gpu_device), draw.to(gpu_device)
        if kind == "avid":
            na.sample_negatives = lambda yy, KK, _i=dd: _i
        else:
            na.multinomial.draw = lambda n, _r=dd: _r.reshape(-1)
        with kernel_log() as log:
            loss, tb = crit(vd, ad, yd)
            loss.backward()
        assert log.launches("xmodal_fused_kernel") == 0 and log.launches("cma_fused_kernel") == 0
        assert log.launches("bank_scores_fwd_kernel") >= 4 and log.launches("bank_scores_bwd_kernel") >= 4
        tag = f"{kind} D {D} step {step}"
        _close(f"{tag} loss", loss.item(), w["loss"], W.CRIT_TOL["loss"])
        _close(f"{tag} Z", float(crit.criterion.avg_exp_score), w["Z"], W.CRIT_TOL["Z"])
        assert set(tb) == set(w["tb"]), (sorted(tb), sorted(w["tb"]))
        for k in sorted(tb):
            _close(f"{tag} {k}", float(tb[k].detach() if torch.is_tensor(tb[k]) else tb[k]), w["tb"][k], W.CRIT_TOL["tb"])
        _close(f"{tag} d loss / d video emb", vd.grad, w["gv"], W.CRIT_TOL["grad"])
        _close(f"{tag} d loss / d audio emb", ad.grad, w["ga"], W.CRIT_TOL["grad"])
        _close(f"{tag} video bank rows", na.view1_mem[yd], w["v1rows"], W.CRIT_TOL["rows"])
        _close(f"{tag} audio bank rows", na.view2_mem[yd], w["v2rows"], W.CRIT_TOL["rows"])
        if step == 0:
            z1 = crit.criterion.avg_exp_score.clone()
        else:
            assert torch.equal(crit.criterion.avg_exp_score, z1)               # Z is carried, not recomputed
    from avid_hip import ops
    ops.check_device_errors(gpu_device)


def test_criterion_never_takes_the_fused_kernel_at_another_width(gpu_device):
    """The stock term sets (what ``fused_ok`` accepts at D = 128) at D = 64 and 256."""
    import criterions
    for D in W.CRIT_WIDTHS:
        v = torch.zeros(2, D, device=gpu_device)
        crit = criterions.AVID(num_data=100, embedding_dim=D, num_negatives=8, device=gpu_device.index)
        assert not crit.nce_average.fused_ok(v, v)
        na = _criterion("cma", D, gpu_device).nce_average
        na.xModalInst, na.wModalPos, na.wModalInst, na.xModalPos = True, True, False, False
        assert not na.fused_ok(v, v)
    crit = criterions.AVID(num_data=100, embedding_dim=128, num_negatives=8, device=gpu_device.index)
    assert crit.nce_average.fused_ok(torch.zeros(2, 128, device=gpu_device), torch.zeros(2, 128, device=gpu_device))


@pytest.mark.parametrize("kind", ["avid", "cma"])
def test_criterion_refuses_a_width_without_a_scores_kernel(kind, gpu_device, kernel_log):
    """embedding_dim = 100: normalize takes it, ``avid_bank_scores_fwd`` has no instance for it — the first forward raises,
    naming the width, before the banks are touched."""
    from avid_hip.lib import AvidHipError
    crit = _criterion(kind, 100, gpu_device)
    na, c = crit.nce_average, W.CRIT[kind]
    g = torch.Generator().manual_seed(100)
    if kind == "cma":
        na.register_buffer("positive_set", torch.from_numpy(W.positive_set(64)).to(gpu_device))
    b1, b2 = na.view1_mem.clone(), na.view2_mem.clone()
    v, a = (torch.randn(c["bs"], 100, generator=g).to(gpu_device).requires_grad_(True) for _ in range(2))
    y = torch.randperm(c["N"], generator=g)[:c["bs"]].to(gpu_device)
    with kernel_log() as log:
        with pytest.raises(AvidHipError, match="D=100"):
            crit(v, a, y)
    assert log.launches("bank_scores") == 0
    assert torch.equal(na.view1_mem, b1) and torch.equal(na.view2_mem, b2)


# ---- h. block edges of the fused kernels (D = 128) --------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 63, 64, 65, 128, 129, 4096])
def test_xmodal_fused_block_edges(K, gpu_device):
    """ops.xmodal_fused splits the K negatives into blocks of 64 (the sample's own row rides in the first): K = 1, a block one row
    short, exactly one block, one row into the second, two blocks, one row into the third, and the reference's default
    ``num_negatives=4096``.  Assertions and tolerances of test_xmodal_fused_vs_unfused_ops_and_fp64."""
    from avid_hip import ops
    bs, N = 3, 300
    c = xmodal_case(bs, K, N)
    b1, b2 = c.v1.to(gpu_device), c.v2.to(gpu_device)
    vd, ad = c.ve.to(gpu_device).requires_grad_(True), c.ae.to(gpu_device).requires_grad_(True)
    ws = ops.xmodal_fused_workspace(gpu_device, bs, K)
    outs = [ops.xmodal_fused(vd, ad, c.y.to(gpu_device), c.idx.to(gpu_device), b1, b2, c.Z.to(gpu_device), 1 / c.T, c.coeff, ws)
            for _ in range(3)]
    total, losses, hats = outs[0]
    assert all(torch.equal(o[0], total) and torch.equal(o[1], losses) and torch.equal(o[2], hats) for o in outs[1:])
    (total * 2.0).backward()
    print(f"K {K}: losses {losses.cpu().numpy()} vs {c.losses}; gradients {relerr(vd.grad, 2.0 * c.gv):.2e} {relerr(ad.grad, 2.0 * c.ga):.2e}")
    np.testing.assert_allclose(losses.cpu().numpy(), c.losses, rtol=2e-6)
    assert relerr(hats[0], c.vh) < 1e-6 and relerr(hats[1], c.ah) < 1e-6
    assert relerr(vd.grad, 2.0 * c.gv) < 2e-5 and relerr(ad.grad, 2.0 * c.ga) < 2e-5
    assert torch.equal(b1.cpu(), c.v1) and torch.equal(b2.cpu(), c.v2)
    ops.check_device_errors(gpu_device)


@pytest.mark.parametrize("P,K,Kw", [(1, 1, 1), (31, 32, 32), (63, 64, 64), (64, 65, 1), (32, 128, 31), (32, 4096, 64)])
def test_cma_fused_block_edges(P, K, Kw, gpu_device):
    """ops.cma_fused splits its 1 + P + K rows into blocks of 64: three rows, exactly one block (Kw = K), exactly two, two rows
    into the third with a single within-modal negative, a ``Kw`` that ends inside a block and one that ends on a block edge
    (1 + 32 + 31 = 64; 1 + 32 + 64 = 97 with K = 4096).  Assertions and tolerances of
    test_cma_fused_vs_fp64_and_the_criterion_it_replaces."""
    from avid_hip import ops
    bs, N = 3, 300
    c = cma_case(bs, P, K, Kw, N)
    b1, b2 = c.v1.to(gpu_device), c.v2.to(gpu_device)
    vd, ad = c.ve.to(gpu_device).requires_grad_(True), c.ae.to(gpu_device).requires_grad_(True)
    ws = ops.cma_fused_workspace(gpu_device, bs, P, K)
    outs = [ops.cma_fused(vd, ad, c.y.to(gpu_device), c.pos.to(gpu_device), c.idx.to(gpu_device), b1, b2, c.Z.to(gpu_device), 1 / c.T,
                          Kw, c.cI, c.cP, ws) for _ in range(3)]
    total, losses, hats = outs[0]
    assert all(torch.equal(o[0], total) and torch.equal(o[1][:7], losses[:7]) and torch.equal(o[2], hats) for o in outs[1:])
    (total * 2.0).backward()
    print(f"P {P} K {K} Kw {Kw}: losses {losses[:7].cpu().numpy()} vs {c.losses}; gradients {relerr(vd.grad, 2.0 * c.gv):.2e} "
          f"{relerr(ad.grad, 2.0 * c.ga):.2e}")
    np.testing.assert_allclose(losses[:7].cpu().numpy(), c.losses, rtol=2e-6)
    assert relerr(hats[0], c.vh) < 1e-6 and relerr(hats[1], c.ah) < 1e-6
    assert relerr(vd.grad, 2.0 * c.gv) < 2e-5 and relerr(ad.grad, 2.0 * c.ga) < 2e-5
    ops.check_device_errors(gpu_device)


# ---- i. nce_loss on the 16-block path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint", [False, True], ids=["two_tensors", "split_scores"])
@pytest.mark.parametrize("bs,Pn,K", [(1, 1, 16385), (16384, 1, 1), (5, 32, 4096), (3, 1, 5462)])
def test_nce_multi_block_edges(bs, Pn, K, joint, gpu_device):
    """avid_nce_fwd with bs * K >= 16384 runs 16 blocks of 1024 threads that keep (row, col) of their elements incrementally
    from stride / K and stride % K (stride = 16384): K larger than the stride, K = 1, a K that divides nothing, and P = 32;
    through two tensors (leading dimension K) and through ``ops.split_scores`` (leading dimension P + K).  Against
    ``O.nce_loss`` in float64 at the tolerances of test_nce_multi_block_path; five calls bit-identical."""
    from avid_hip import ops
    gen = torch.Generator().manual_seed(bs + Pn + K)
    base = torch.rand(bs, Pn + K, generator=gen) * 16 - 8
    Z = torch.tensor(0.37)
    ref = base.double().requires_grad_(True)
    want, _ = O.nce_loss(ref[:, :Pn], ref[:, Pn:], Z.double())
    want.backward()
    Zd = Z.to(gpu_device)
    if joint:
        s = base.to(gpu_device).requires_grad_(True)
        losses = []
        for _ in range(5):
            pos, neg = ops.split_scores(s * 1.0, Pn)
            losses.append(ops.nce_loss(pos, neg, Zd))
        assert type(losses[-1].grad_fn).__name__.startswith("_NCELossJoint")
        losses[-1].backward()
        grad = s.grad
    else:
        sp = base[:, :Pn].contiguous().to(gpu_device).requires_grad_(True)
        sn = base[:, Pn:].contiguous().to(gpu_device).requires_grad_(True)
        losses = [ops.nce_loss(sp, sn, Zd) for _ in range(5)]
        losses[-1].backward()
        grad = torch.cat([sp.grad, sn.grad], 1)
    print(f"bs {bs} P {Pn} K {K} joint {joint}: loss {losses[0].item()!r} vs {float(want)!r}")
    np.testing.assert_allclose(losses[0].item(), float(want), rtol=2e-6)
    assert all(torch.equal(l, losses[0]) for l in losses[1:])
    np.testing.assert_allclose(grad.cpu().numpy(), ref.grad.float().numpy(), rtol=2e-5, atol=1e-9)
