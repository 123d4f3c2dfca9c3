"""Linear SVM evaluation on the GPU (csrc/svm.hip, ops.svm_scores / svm_xt / svm_fit, parallel.SVMEval) against the float64
restatement tests/_svm_ref.py.

1. Exact: on lattice inputs every product and sum is exact in float32, so the two products equal float64 bit for bit — at
   every tile, slice, remainder and class-block edge.
2. Bounds: on Gaussian data they stay within the per-element bounds derived from the summation structure.
3. Determinism: run to run, under CU budgets, and for a row block scored alone.
4. Solver: the float64 gradient at the returned iterate meets the stopping rule up to the float32 evaluation bound, the iterate
   is within |g| + |g*| of the reference optimum (1-strong convexity: no margin), objective, flags, warm start.
5. Predictions on held-out rows.  6. Guard bands.  7. ``SVMEval`` end to end around both towers."""
import numpy as np
import pytest
import torch

import _audio_downstream as AD
import _svm_ref as R
from _guards import FILLS, guarded
from _inference_probe import wrapper

pytestmark = pytest.mark.gpu
S = R.SLICE


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    """The float32 bits with the sign of zero dropped (a float64 sum of -0.0 products is +0.0 or -0.0 by the order)."""
    return (np.asarray(t, np.float32) + np.float32(0.0)).view(np.uint32)


def _scores_inputs(N, F, C, seed, lattice):
    rng = np.random.default_rng(seed)
    if lattice:
        return R.lattice(rng, (N, F), -4, 4, 8), R.lattice(rng, (C, F), -8, 8, 16), R.lattice(rng, (C,), -12, 12, 4)
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((N, F), (C, F), (C,)))


def _xt_inputs(N, F, C, seed, lattice):
    rng = np.random.default_rng(seed)
    if lattice:
        return R.lattice(rng, (N, F), -4, 4, 8), R.lattice(rng, (N, C), -8, 8, 16)
    return rng.standard_normal((N, F)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)


# ---- 1. exact ----------------------------------------------------------------------------------------------------------------
# every N edge of the 64-row tile, every F edge (1, a remainder of 1, whole stages, a remainder of 8 in a 32-step stage), every C edge
SCORES_SHAPES = [(1, 1, 1), (63, 33, 3), (64, 512, 50), (65, 1000, 64), (193, 33, 65), (65, 512, 101), (193, 1, 50), (64, 1000, 3)]
XT_SHAPES = [(S - 1, 33, 3), (S, 1, 1), (S + 1, 1000, 65), (2 * S + 7, 512, 50), (S + 1, 33, 101), (2 * S + 7, 33, 64),
             (S - 1, 512, 64), (S, 1000, 50)]


@pytest.mark.parametrize("N,F,C", SCORES_SHAPES, ids=["x".join(map(str, s)) for s in SCORES_SHAPES])
def test_scores_are_exact_on_lattice_inputs(gpu_device, N, F, C):
    from avid_hip import ops
    X, W, b = _scores_inputs(N, F, C, N + F + C, True)
    z = ops.svm_scores(_dev(X, gpu_device), _dev(W, gpu_device), _dev(b, gpu_device)).cpu().numpy()
    assert z.shape == (N, C) and np.array_equal(_bits(z), _bits(R.scores64(X, W, b)))
    z0 = ops.svm_scores(_dev(X, gpu_device), _dev(W, gpu_device)).cpu().numpy()
    assert np.array_equal(_bits(z0), _bits(R.scores64(X, W)))


@pytest.mark.parametrize("N,F,C", XT_SHAPES, ids=["x".join(map(str, s)) for s in XT_SHAPES])
def test_xt_is_exact_on_lattice_inputs(gpu_device, N, F, C):
    from avid_hip import ops
    X, D = _xt_inputs(N, F, C, N + F + C, True)
    g, gb = ops.svm_xt(_dev(X, gpu_device), _dev(D, gpu_device))
    want_g, want_gb = R.xt64(X, D)
    assert g.shape == (C, F) and gb.shape == (C,)
    assert np.array_equal(_bits(g.cpu().numpy()), _bits(want_g)) and np.array_equal(_bits(gb.cpu().numpy()), _bits(want_gb))
    g2, none = ops.svm_xt(_dev(X, gpu_device), _dev(D, gpu_device), colsum=False)
    assert none is None and torch.equal(g2, g)


# ---- 2. bounds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F,C", [(193, 1000, 65), (65, 33, 3)])
def test_scores_stay_within_the_derived_bound(gpu_device, N, F, C):
    from avid_hip import ops
    X, W, b = _scores_inputs(N, F, C, 7, False)
    z = ops.svm_scores(_dev(X, gpu_device), _dev(W, gpu_device), _dev(b, gpu_device)).cpu().numpy().astype(np.float64)
    ratio = np.abs(z - R.scores64(X, W, b)) / R.scores_bound(X, W, b)
    print(f"scores {N}x{F}x{C}: largest error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("N,F,C", [(2 * S + 7, 33, 65), (S + 1, 1000, 3)])
def test_xt_stays_within_the_derived_bound(gpu_device, N, F, C):
    from avid_hip import ops
    X, D = _xt_inputs(N, F, C, 8, False)
    g, gb = ops.svm_xt(_dev(X, gpu_device), _dev(D, gpu_device))
    (want_g, want_gb), (bg, bgb) = R.xt64(X, D), R.xt_bound(X, D)
    rg = np.abs(g.cpu().numpy().astype(np.float64) - want_g) / bg
    rb = np.abs(gb.cpu().numpy().astype(np.float64) - want_gb) / bgb
    print(f"xt {N}x{F}x{C}: largest error / bound {rg.max():.3f} (tiles), {rb.max():.3f} (column sums)")
    assert rg.max() <= 1.0 and rb.max() <= 1.0


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------
def test_same_bits_from_run_to_run_and_under_cu_budgets(gpu_device):
    from avid_hip import ops
    X, W, b = (_dev(a, gpu_device) for a in _scores_inputs(2 * S + 7, 100, 65, 9, False))
    D = _dev(_xt_inputs(2 * S + 7, 100, 65, 10, False)[1], gpu_device)
    z, (g, gb) = ops.svm_scores(X, W, b), ops.svm_xt(X, D)
    z2, (g2, gb2) = ops.svm_scores(X, W, b), ops.svm_xt(X, D)
    assert torch.equal(z, z2) and torch.equal(g, g2) and torch.equal(gb, gb2)
    try:
        for cus in (8, 24):
            assert ops.set_cu_budget(cus) == cus
            zb, (gbud, gbb) = ops.svm_scores(X, W, b), ops.svm_xt(X, D)
            assert torch.equal(z, zb) and torch.equal(g, gbud) and torch.equal(gb, gbb), cus
    finally:
        ops.set_cu_budget(0)


@pytest.mark.parametrize("F,lo,hi", [(33, 5, 70), (512, 64, 129)])
def test_a_row_block_scored_alone_has_the_bits_it_has_in_the_matrix(gpu_device, F, lo, hi):
    from avid_hip import ops
    X, W, b = (_dev(a, gpu_device) for a in _scores_inputs(193, F, 50, 11, False))
    z = ops.svm_scores(X, W, b)
    block = X[lo:hi]
    assert block.is_contiguous() and torch.equal(ops.svm_scores(block, W, b), z[lo:hi])
    assert torch.equal(ops.svm_scores(block.clone(), W, b), z[lo:hi])


# ---- 4. the solver -------------------------------------------------------------------------------------------------------------
_SOLVED = {}


def _reference(name):
    """The case, its float64 optimum and the quantities the checks share — computed once."""
    if name not in _SOLVED:
        case = R.solver_case(name)
        Wa, iters, conv = R.newton_solve(case["X"], case["labels"], case["C"], case["cost"], case["pos_weight"], case["s"])
        assert conv.all()
        Xa, Y = R.augmented(case["X"], case["s"]), R.targets(case["labels"], case["C"])
        Cst = R.costs(case["labels"], case["C"], case["cost"], case["pos_weight"])
        _SOLVED[name] = (case, Wa, Xa, Y, Cst)
    return _SOLVED[name]


def _fit(case, dev, **kw):
    from avid_hip import ops
    pw = None if case["pos_weight"] is None else _dev(case["pos_weight"], dev)
    return ops.svm_fit(_dev(case["X"], dev), _dev(case["labels"], dev), case["C"], cost=case["cost"], pos_weight=pw,
                       intercept_scaling=case["s"], **kw)


def _iterate(coef, icpt, s):
    return np.concatenate([coef.cpu().numpy().astype(np.float64), icpt.cpu().numpy().astype(np.float64)[:, None] / s], 1)


@pytest.mark.parametrize("name", sorted(R.SOLVER_CASES))
def test_solver_meets_the_stopping_rule_and_the_reference_optimum(gpu_device, name):
    tol = 1e-4
    case, Wstar, Xa, Y, Cst = _reference(name)
    coef, icpt, info = _fit(case, gpu_device, tol=tol)
    assert coef.shape == (case["C"], case["X"].shape[1]) and icpt.shape == (case["C"],) and coef.dtype == icpt.dtype == torch.float32
    assert all(info[k].is_cuda and info[k].shape == (case["C"],) for k in ("objective", "grad_norm", "grad_norm0", "iterations", "converged"))
    Wa = _iterate(coef, icpt, case["s"])
    g = np.linalg.norm(R.gradient(Wa, Xa, Y, Cst), axis=1)
    g0 = np.linalg.norm(R.gradient(np.zeros_like(Wa), Xa, Y, Cst), axis=1)
    gstar = np.linalg.norm(R.gradient(Wstar, Xa, Y, Cst), axis=1)
    E = R.gradient_eval_bound(coef.cpu().numpy(), icpt.cpu().numpy(), case["X"], case["labels"], case["cost"], case["pos_weight"], case["s"])
    dist = np.linalg.norm(Wa - Wstar, axis=1)
    print(f"{name}: |g| / |g0| <= {(g / g0).max():.3e}, E / |g0| <= {(E / g0).max():.3e}, |wa - wa*| <= {dist.max():.3e} "
          f"(|g| + |g*| >= {(g + gstar).min():.3e}), Newton steps {info['iterations'].tolist()[:8]}")
    assert (g <= tol * g0 + E).all()
    assert (dist <= g + gstar).all()
    assert bool(info["converged"].all()) and int(info["iterations"].max()) <= 50
    # what the solver reports about itself
    assert np.abs(info["grad_norm"].cpu().numpy() - g).max() <= E.max() and np.abs(info["grad_norm0"].cpu().numpy() / g0 - 1).max() <= 1e-4
    f64 = R.objective(Wa, Xa, Y, Cst)
    fb = R.objective_eval_bound(coef.cpu().numpy(), icpt.cpu().numpy(), case["X"], case["labels"], case["cost"], case["pos_weight"], case["s"])
    assert info["objective"].dtype == torch.float64 and (np.abs(info["objective"].cpu().numpy() - f64) <= fb).all()
    # a warm start from the solution returns at once
    coef2, icpt2, info2 = _fit(case, gpu_device, tol=tol, init=(coef, icpt))
    assert int(info2["iterations"].sum()) == 0 and bool(info2["converged"].all())
    assert torch.equal(coef2, coef) and torch.equal(icpt2, icpt)


def test_solver_flags_what_it_did_not_finish_and_reports_bad_labels(gpu_device):
    from avid_hip import ops
    case = R.solver_case("n193_f33_c3")
    coef, icpt, info = _fit(case, gpu_device, max_iter=1)
    assert not bool(info["converged"].any()) and info["iterations"].tolist() == [1, 1, 1]     # flagged, not raised
    coef0, icpt0, info0 = _fit(case, gpu_device, max_iter=0)
    assert not coef0.any() and not icpt0.any() and torch.equal(info0["grad_norm"], info0["grad_norm0"])
    labels = case["labels"].copy()
    labels[17] = 3
    with pytest.raises(ops.LabelError):
        ops.svm_fit(_dev(case["X"], gpu_device), _dev(labels, gpu_device), 3)


# ---- 5. predictions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SOLVER_CASES))
def test_decision_values_and_argmax_on_held_out_rows(gpu_device, name):
    from avid_hip import ops
    case, Wstar, _, _, _ = _reference(name)
    coef, icpt, _ = _fit(case, gpu_device)
    Xt = R.augmented(case["X_test"], case["s"])
    z = ops.svm_scores(_dev(case["X_test"], gpu_device), coef, icpt).cpu().numpy().astype(np.float64)
    want = Xt @ Wstar.T
    dw = np.linalg.norm(_iterate(coef, icpt, case["s"]) - Wstar, axis=1)
    bound = np.linalg.norm(Xt, axis=1)[:, None] * dw[None, :] + R.scores_bound(case["X_test"], coef.cpu().numpy(), icpt.cpu().numpy(), extra=1)
    assert (np.abs(z - want) <= bound).all()
    top = np.sort(want, 1)
    sure = top[:, -1] - top[:, -2] > 2 * bound.max(1)
    print(f"{name}: {int((~sure).sum())} of {len(sure)} held-out rows exempt")
    assert (~sure).mean() <= 0.10 and np.array_equal(z.argmax(1)[sure], want.argmax(1)[sure])


# ---- 6. guard bands ------------------------------------------------------------------------------------------------------------
def _guard_products(dev, P):
    from avid_hip import ops
    X, W, b = (P(_dev(a, dev)) for a in _scores_inputs(S + 1, 33, 65, 12, False))
    D = P(_dev(_xt_inputs(S + 1, 33, 65, 13, False)[1], dev))
    g, gb = ops.svm_xt(X, D)
    return {"z": ops.svm_scores(X, W, b), "g": g, "gb": gb}


def _guard_fit(dev, P):
    from avid_hip import ops
    case = R.solver_case("n193_f33_c3")
    coef, icpt, info = ops.svm_fit(P(_dev(case["X"], dev)), P(_dev(case["labels"], dev)), case["C"], cost=case["cost"],
                                   intercept_scaling=case["s"])
    return {"coef": coef, "intercept": icpt, **info}


@pytest.mark.parametrize("case", [_guard_products, _guard_fit], ids=["products", "fit"])
def test_svm_ops_under_guards(gpu_device, case):
    """tests/test_gpu_guards.py's rule: no byte of a guard band changes with every workspace exactly
    avid_svm_workspace_bytes, and the results are the same bits under both fills of unwritten memory and without guards."""
    from avid_hip import lib
    plain = {k: v.clone() for k, v in case(gpu_device, lambda t: t).items()}
    runs = []
    for fill in FILLS:
        with guarded(fill) as g:
            res = case(gpu_device, g.place)
            torch.cuda.synchronize()
            g.check()
            runs.append({k: v.clone() for k, v in res.items()})
        shape = (S + 1, 33, 65) if case is _guard_products else (193, 33, 3)
        need = int(lib.raw("avid_svm_workspace_bytes")(*shape))
        assert g.workspaces and {w[0] for w in g.workspaces} == {need} and need in g.size_values
    for k in plain:
        assert torch.equal(runs[0][k], runs[1][k]), f"'{k}' depends on unwritten memory"
        assert torch.equal(runs[0][k], plain[k]), f"'{k}' differs under guards"


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------
def _end_to_end(dev, model, batches, labels, query, query_labels, n_classes):
    from avid_hip import parallel
    ev = parallel.SVMEval(model, n_classes=n_classes, cost=0.5)
    for x, l in zip(batches, labels):
        ev.add_train(x, l, clips_per_sample=2)
    ev.fit()
    assert bool(ev.info["converged"].all())
    z = ev.decision_function(query)
    B = query_labels.shape[0]
    assert z.shape == (2 * B, n_classes) and z.dtype == torch.float32
    out = ev.evaluate(query, query_labels, clips_per_sample=2)
    assert all(out[k].is_cuda and out[k].dtype == torch.int64 for k in ("n", "top1_hits", "top5_hits"))
    avg = z.view(B, 2, n_classes).mean(1)
    top5 = avg.topk(min(5, n_classes), dim=1).indices
    assert (int(out["n"]), int(out["top1_hits"]), int(out["top5_hits"])) == \
        (B, int((avg.argmax(1) == query_labels).sum()), int((top5 == query_labels[:, None]).any(1).sum()))
    # a state_dict round trip reproduces the scores bit for bit
    ev2 = parallel.SVMEval(model, n_classes=n_classes)
    ev2.load_state_dict({k: v.clone() for k, v in ev.state_dict().items()})
    assert torch.equal(ev2.decision_function(query), z)
    # passing features equals passing clips
    infer = parallel.Inference(model)

    def feats(x):
        x = x.flatten(0, 1) if x.dim() == 6 else x
        return infer(x.contiguous()).flatten(1)
    evf = parallel.SVMEval(None, n_classes=n_classes, cost=0.5)
    for x, l in zip(batches, labels):
        evf.add_train(feats(x), l, clips_per_sample=2)
    evf.fit()
    assert torch.equal(evf.coef, ev.coef) and torch.equal(evf.intercept, ev.intercept)
    assert torch.equal(evf.decision_function(feats(query)), z)
    assert all(mod.training for mod in model.modules())


def test_svmeval_around_the_video_tower(gpu_device):
    """R2Plus1D-18 on 3x8x48x48 clips, two clips per sample: two training batches of 6 samples, one query batch of 5."""
    m = wrapper(gpu_device, seed=31).feature_extractor
    gen = torch.Generator().manual_seed(32)
    batches = [torch.randn((6, 2, 3, 8, 48, 48), generator=gen).to(gpu_device) for _ in range(2)]
    labels = [torch.randint(0, 4, (6,), generator=gen).to(gpu_device) for _ in range(2)]
    query, ql = torch.randn((5, 2, 3, 8, 48, 48), generator=gen).to(gpu_device), torch.randint(0, 4, (5,), generator=gen).to(gpu_device)
    _end_to_end(gpu_device, m, batches, labels, query, ql, 4)


def test_svmeval_around_the_audio_tower(gpu_device):
    """Conv2D on 1x64x65 spectrograms, two clips per sample, a sample's clips adjacent (the flat form)."""
    m = AD.tower_model().to(gpu_device).train()
    gen = torch.Generator().manual_seed(33)
    batches = [torch.randn((12, 1, 64, 65), generator=gen).to(gpu_device) for _ in range(2)]
    labels = [torch.randint(0, 3, (6,), generator=gen).to(gpu_device) for _ in range(2)]
    query, ql = torch.randn((10, 1, 64, 65), generator=gen).to(gpu_device), torch.randint(0, 3, (5,), generator=gen).to(gpu_device)
    _end_to_end(gpu_device, m, batches, labels, query, ql, 3)
