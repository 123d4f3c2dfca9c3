"""Linear SVM evaluation without a GPU: the float64 restatement the kernels and the solver are held to (tests/_svm_ref.py)
against a closed form, its convergence on every input the GPU tests use, the float32 restatements against the derived bounds
(and four planted faults far outside them), the C ABI's declarations and refusals, and ``SVMEval``'s host logic."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _svm_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, SHAPE = -1, -2
NAMES = ("avid_svm_workspace_bytes", "avid_svm_scores", "avid_svm_xt", "avid_svm_hinge", "avid_svm_loss")


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_reference_reaches_the_ridge_closed_form():
    """With a cost so small that every margin stays active the loss is a plain sum of squares: the optimum is the ridge
    solution (I + 2 c X~^T X~)^-1 2 c X~^T y."""
    rng = np.random.default_rng(3)
    X, labels, c, s = rng.standard_normal((60, 8)), rng.integers(0, 4, 60), 1e-3, 2.0
    Xa, Y = R.augmented(X, s), R.targets(labels, 4)
    ridge = np.linalg.solve(np.eye(9) + 2 * c * Xa.T @ Xa, 2 * c * Xa.T @ Y).T
    assert (1.0 - Y * (Xa @ ridge.T) > 0).all(), "the inputs were meant to keep every margin active"
    Wa, iters, conv = R.newton_solve(X, labels, 4, cost=c, s=s)
    assert conv.all() and np.abs(Wa - ridge).max() <= 1e-12
    # ... and a class weight scales the positive rows' cost
    pw = np.array([1.0, 3.0, 1.0, 0.5])
    Cst = R.costs(labels, 4, c, pw)
    Wp, _, conv = R.newton_solve(X, labels, 4, cost=c, pos_weight=pw, s=s)
    for k in range(4):
        want = np.linalg.solve(np.eye(9) + 2 * (Xa * Cst[:, k:k + 1]).T @ Xa, 2 * Xa.T @ (Cst[:, k] * Y[:, k]))
        assert np.abs(Wp[k] - want).max() <= 1e-12
    assert conv.all()


def test_gradient_and_hessian_are_the_objectives():
    rng = np.random.default_rng(4)
    X, labels = rng.standard_normal((40, 5)), rng.integers(0, 3, 40)
    Xa, Y, Cst = R.augmented(X, 1.5), R.targets(labels, 3), R.costs(labels, 3, 0.7, np.array([2.0, 1.0, 1.0]))
    Wa = 0.3 * rng.standard_normal((3, 6))
    g = R.gradient(Wa, Xa, Y, Cst)
    for c in range(3):
        for j in range(6):
            e = np.zeros((3, 6))
            e[c, j] = 1e-6
            num = (R.objective(Wa + e, Xa, Y, Cst)[c] - R.objective(Wa - e, Xa, Y, Cst)[c]) / 2e-6
            assert abs(num - g[c, j]) <= 1e-6 * max(1.0, abs(g[c, j]))
        H = R.hessian(Wa[c], Xa, Y[:, c], Cst[:, c])
        assert np.allclose(H, H.T) and np.linalg.eigvalsh(H).min() >= 1.0 - 1e-12      # 1-strongly convex


@pytest.mark.parametrize("name", sorted(R.SOLVER_CASES))
def test_reference_converges_on_the_gpu_tests_inputs(name):
    """... within its caps, the active set at the optimum is mixed, and the held-out rows the prediction test may exempt
    stay under its cap by the reference alone: with |dwa_c| <= tol |g_c(0)| + E_c + |g*_c| (what the solver test
    asserts of the device's iterate) fewer than 10 % of the rows have a top-two gap within twice the decision bound."""
    case, tol = R.solver_case(name), 1e-4
    C_, s = case["C"], case["s"]
    Wa, iters, conv = R.newton_solve(case["X"], case["labels"], C_, case["cost"], case["pos_weight"], s)
    assert conv.all() and iters.max() <= 50
    Xa, Y = R.augmented(case["X"], s), R.targets(case["labels"], C_)
    Cst = R.costs(case["labels"], C_, case["cost"], case["pos_weight"])
    active = (1.0 - Y * (Xa @ Wa.T) > 0).mean(0)
    assert (active > 0.02).all() and (active < 0.98).all()
    if name.endswith("absent"):
        assert (Y[:, 3] < 0).all()
    g0 = np.linalg.norm(R.gradient(np.zeros_like(Wa), Xa, Y, Cst), axis=1)
    gs = np.linalg.norm(R.gradient(Wa, Xa, Y, Cst), axis=1)
    coef, icpt = Wa[:, :-1].astype(np.float32), (Wa[:, -1] * s).astype(np.float32)
    E = R.gradient_eval_bound(coef, icpt, case["X"], case["labels"], case["cost"], case["pos_weight"], s)
    assert (E <= 1e-4 * g0).all()                       # the float32 evaluation is not what the tolerance is spent on
    Xt = R.augmented(case["X_test"], s)
    bound = (np.linalg.norm(Xt, axis=1)[:, None] * (tol * g0 + E + gs)[None, :]
             + R.scores_bound(case["X_test"], coef, icpt, extra=1)).max(1)
    top = np.sort(Xt @ Wa.T, 1)
    exempt = (top[:, -1] - top[:, -2] <= 2 * bound).mean()
    assert exempt <= 0.10, exempt


# ---- the float32 restatements against the bounds ------------------------------------------------------------------------------
def test_scores_restatement_holds_the_bound_and_the_faults_do_not():
    rng = np.random.default_rng(5)
    X, W, b = (rng.standard_normal(sh).astype(np.float32) for sh in ((70, 33), (65, 33), (65,)))
    want, bound = R.scores64(X, W, b), R.scores_bound(X, W, b)
    ratio = np.abs(R.scores_f32(X, W, b).astype(np.float64) - want) / bound
    assert ratio.max() <= 1.0
    for fault in ("remainder", "bias", "pitch"):
        worst = (np.abs(R.scores_f32(X, W, b, fault=fault).astype(np.float64) - want) / bound).max()
        assert worst >= 10.0, (fault, worst)
    assert R.chain_len(33) == 17 and R.chain_len(4) == 2 and R.chain_len(3) == 2 and R.chain_len(1) == 1


def test_xt_restatement_holds_the_bound_and_a_dropped_slice_does_not():
    rng = np.random.default_rng(6)
    N = 2 * R.SLICE + 7
    X, D = rng.standard_normal((N, 33)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    (g64, gb64), (bg, bgb) = R.xt64(X, D), R.xt_bound(X, D)
    g, gb = R.xt_f32(X, D)
    assert (np.abs(g.astype(np.float64) - g64) <= bg).all() and (np.abs(gb.astype(np.float64) - gb64) <= bgb).all()
    g, gb = R.xt_f32(X, D, fault="slice")
    assert (np.abs(g.astype(np.float64) - g64) / bg).max() >= 10.0 and (np.abs(gb.astype(np.float64) - gb64) / bgb).max() >= 10.0


def test_lattice_inputs_are_exact_in_float32():
    rng = np.random.default_rng(7)
    X, W, b = R.lattice(rng, (65, 1000), -4, 4, 8), R.lattice(rng, (3, 1000), -8, 8, 16), R.lattice(rng, (3,), -8, 8, 4)
    assert np.array_equal(R.scores_f32(X, W, b).astype(np.float64), R.scores64(X, W, b))
    D = R.lattice(rng, (65, 3), -8, 8, 16)
    g, gb = R.xt_f32(X, D)
    assert np.array_equal(g.astype(np.float64), R.xt64(X, D)[0]) and np.array_equal(gb.astype(np.float64), R.xt64(X, D)[1])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_sized():
    from avid_hip import lib, ops
    header = open(os.path.join(REPO, "include", "avid_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SIGNATURES and hasattr(lib.raw(name), "argtypes")
    assert lib.version() >= 173
    assert lib.SIGNATURES["avid_svm_workspace_bytes"] == (C.c_size_t, [C.c_int64, C.c_int, C.c_int])
    assert [len(lib.SIGNATURES[n][1]) for n in NAMES[1:]] == [8, 10, 10, 13]
    assert "AVID_DEVERR_SVM_LABEL 256" in header and ops.DeviceErrors._MSG[256].startswith("svm")
    need = lib.raw("avid_svm_workspace_bytes")
    assert ops.SVM_SLICE_ROWS == R.SLICE == 512
    # slices of 512 rows: column partials (double) + partial tiles (float); the ladder's partial sums where they are larger
    assert need(16000, 8192, 50) == 32 * 50 * (8 + 4 * 8192)
    assert need(513, 330, 3) == 2 * 3 * (8 + 4 * 330) and need(512, 330, 3) == 3 * (8 + 4 * 330)
    assert need(1000, 4, 7) == 4 * 16 * 7 * 8
    assert need(0, 4, 4) == 0 and need(1 << 31, 4, 4) == 0 and need(4, 0, 4) == 0 and need(4, 4, 0) == 0
    assert need((1 << 31) - 1, 8192, 1) > (1 << 35)


def test_entry_points_refuse_before_any_launch():
    """No device here: a launch would come back as a HIP error (-3), a refusal is its own code and message."""
    from avid_hip import lib
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    need = lib.raw("avid_svm_workspace_bytes")(100, 64, 3)

    def scores(N=100, F=64, C_=3, x=p, w=p, z=p):
        return lib.raw("avid_svm_scores")(N, F, C_, x, w, None, z, None)

    def xt(N=100, F=64, C_=3, x=p, d=p, g=p, ws=p, nb=need):
        return lib.raw("avid_svm_xt")(N, F, C_, x, d, g, None, ws, nb, None)

    def hinge(N=100, C_=3, z=p, labels=p, cost=1.0, out=p):
        return lib.raw("avid_svm_hinge")(N, C_, z, labels, cost, None, None, out, None, None)

    def loss(N=100, C_=3, K=1, z=p, zd=None, labels=p, cost=1.0, out=p, ws=p, nb=need):
        return lib.raw("avid_svm_loss")(N, C_, K, z, zd, labels, cost, None, out, ws, nb, None, None)

    for fn, args in ((scores, ("x", "w", "z")), (xt, ("x", "d", "g", "ws")), (hinge, ("z", "labels", "out")),
                     (loss, ("z", "labels", "out", "ws"))):
        for a in args:
            assert fn(**{a: None}) == BADARG and lib.last_error(), (fn.__name__, a)
        for bad in (dict(N=0), dict(N=1 << 31), dict(C_=0)):
            assert fn(**bad) == SHAPE and "outside" in lib.last_error(), (fn.__name__, bad)
    assert scores(F=0) == SHAPE and xt(F=0) == SHAPE
    assert xt(nb=need - 1) == BADARG and "workspace" in lib.last_error()
    assert loss(nb=7) == BADARG and "workspace" in lib.last_error()
    assert loss(K=0) == BADARG and loss(K=17, zd=p) == BADARG and loss(K=2) == BADARG
    assert hinge(cost=0.0) == BADARG and loss(cost=float("nan")) == BADARG


def test_ops_refuse_cpu_mistyped_and_strided_tensors():
    from avid_hip import ops
    from avid_hip.lib import AvidHipError
    x, w, d = torch.zeros(8, 4), torch.zeros(3, 4), torch.zeros(8, 3)
    labels = torch.zeros(8, dtype=torch.int64)
    for call in (lambda: ops.svm_scores(x, w), lambda: ops.svm_xt(x, d), lambda: ops.svm_fit(x, labels, 3)):
        with pytest.raises(AvidHipError, match="device tensor"):
            call()
    # the dtype and layout checks, reached with tensors that claim to live on the device: refused before any launch
    for call in (lambda: ops.svm_scores(_Fake(torch.float64), _Fake(torch.float64)),
                 lambda: ops.svm_xt(_Fake(torch.float32), _Fake(torch.float16)),
                 lambda: ops.svm_fit(_Fake(torch.float64), labels, 3)):
        with pytest.raises(AvidHipError, match="must be torch.float32"):
            call()
    for call in (lambda: ops.svm_scores(_Fake(torch.float32, contiguous=False), _Fake(torch.float32)),
                 lambda: ops.svm_scores(_Fake(torch.float32), _Fake(torch.float32, contiguous=False)),
                 lambda: ops.svm_xt(_Fake(torch.float32), _Fake(torch.float32, contiguous=False)),
                 lambda: ops.svm_fit(_Fake(torch.float32, contiguous=False), labels, 3)):
        with pytest.raises(AvidHipError, match="contiguous"):
            call()
    with pytest.raises(AvidHipError, match="labels"):
        ops.svm_fit(_Fake(torch.float32), labels[:4], 3)


class _Fake(torch.Tensor):
    """A tensor that claims to live on the device: reaches the dtype and layout checks of the ops without one."""
    @staticmethod
    def __new__(cls, dtype, contiguous=True):
        t = torch.zeros(4, 4, dtype=dtype)
        return torch.Tensor._make_subclass(cls, t if contiguous else t.t()[:, ::2])

    def __init__(self, dtype, contiguous=True):
        pass

    @property
    def is_cuda(self):
        return True


def test_kernels_carry_no_scratch():
    from tools_path import kernel_table
    rows = {r["name"]: r for r in kernel_table() if r["name"].startswith("svm_")}
    assert sorted(rows) == ["svm_colsum_kernel", "svm_gemm_kernel<false>", "svm_gemm_kernel<true>", "svm_hinge_kernel",
                            "svm_loss_finish_kernel", "svm_loss_kernel", "svm_reduce_kernel"]
    for r in rows.values():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0 and not r["uses_dynamic_stack"], r


# ---- SVMEval's host logic over the restatement ----------------------------------------------------------------------------------
@pytest.fixture
def ref_ops(monkeypatch):
    """``ops.svm_fit`` / ``ops.svm_scores`` replaced by the float64 restatement on CPU tensors; the calls are recorded."""
    from avid_hip import ops
    calls = []

    def fit(X, labels, n_classes, cost=1.0, pos_weight=None, intercept_scaling=1.0, tol=1e-4, max_iter=100, init=None):
        calls.append(("fit", X.clone(), labels.clone(), n_classes, cost, intercept_scaling, tol, init))
        Wa, iters, conv = R.newton_solve(X.numpy(), labels.numpy(), n_classes, cost, pos_weight, intercept_scaling)
        return (torch.from_numpy(Wa[:, :-1].astype(np.float32)), torch.from_numpy((Wa[:, -1] * intercept_scaling).astype(np.float32)),
                {"iterations": torch.from_numpy(iters), "converged": torch.from_numpy(conv)})

    def scores(x, w, bias=None):
        calls.append(("scores", x.clone()))
        return torch.from_numpy(R.scores64(x.numpy(), w.numpy(), bias.numpy()).astype(np.float32))

    monkeypatch.setattr(ops, "svm_fit", fit)
    monkeypatch.setattr(ops, "svm_scores", scores)
    return calls


def test_svmeval_trains_on_clip_rows_and_averages_clip_scores(ref_ops):
    from avid_hip import parallel
    X, labels = R.blobs(60, 12, 4, seed=11, sep=3.0)
    X = torch.from_numpy(X * 3.0 + 5.0)                              # off zero and off unit scale: standardising matters
    sample_labels = torch.from_numpy(labels[::2].copy())             # 30 samples x 2 clips, a sample's clips adjacent
    ev = parallel.SVMEval(n_classes=4, cost=0.5, intercept_scaling=2.0)
    ev.add_train(X[:20], sample_labels[:10], clips_per_sample=2)
    ev.add_train(X[20:], sample_labels[10:].to(torch.int32), clips_per_sample=2)
    assert ev.fit() is ev
    kind, Xs, ys, n_classes, cost, s, tol, init = ref_ops[0]
    assert (kind, n_classes, cost, s, tol, init) == ("fit", 4, 0.5, 2.0, 1e-4, None)
    assert torch.equal(ys, sample_labels.repeat_interleave(2)) and ys.dtype == torch.int64
    mean, std = X.mean(0), X.std(0, unbiased=False)
    assert torch.equal(ev.mean, mean) and torch.equal(ev.std, std) and torch.equal(Xs, (X - mean) / std)
    q = X[:14]
    z = ev.decision_function(q)
    assert z.shape == (14, 4) and torch.equal(ref_ops[1][1], (q - mean) / std)
    out = ev.evaluate(q, sample_labels[:7], clips_per_sample=2)
    avg = z.view(7, 2, 4).mean(1)
    assert int(out["n"]) == 7 and out["n"].dtype == torch.int64
    assert int(out["top1_hits"]) == int((avg.argmax(1) == sample_labels[:7]).sum())
    assert int(out["top5_hits"]) == 7                                # four classes: every label is among the best five
    with pytest.raises(ValueError, match="multiple of clips_per_sample"):
        ev.evaluate(X[:13], sample_labels[:7], clips_per_sample=2)
    with pytest.raises(ValueError, match="labels"):
        ev.evaluate(q, sample_labels[:14].float(), clips_per_sample=1)
    # the state: coef, intercept, mean, std — and nothing else is needed to score
    sd = ev.state_dict()
    assert sorted(sd) == ["coef", "intercept", "mean", "std"]
    ev2 = parallel.SVMEval(n_classes=4)
    ev2.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert torch.equal(ev2.decision_function(q), z)
    with pytest.raises(ValueError, match="mean and std"):
        parallel.SVMEval(n_classes=4, standardize=False).load_state_dict(sd)
    with pytest.raises(ValueError, match="classes"):
        parallel.SVMEval(n_classes=5).load_state_dict(sd)


def test_svmeval_without_standardising_and_what_it_refuses(ref_ops):
    from avid_hip import parallel
    X, labels = R.blobs(40, 6, 3, seed=12)
    X, labels = torch.from_numpy(X), torch.from_numpy(labels)
    ev = parallel.SVMEval(n_classes=3, standardize=False)
    ev.add_train(X, labels)
    ev.fit()
    assert ev.mean is None and torch.equal(ref_ops[0][1], X) and sorted(ev.state_dict()) == ["coef", "intercept"]
    # a constant feature keeps its scale (its deviation is zero)
    Xc = X.clone()
    Xc[:, 2] = 4.0
    ev = parallel.SVMEval(n_classes=3)
    ev.add_train(Xc, labels)
    ev.fit()
    assert float(ev.std[2]) == 1.0 and torch.isfinite(ref_ops[-1][1]).all() and float(ref_ops[-1][1][:, 2].abs().max()) == 0.0
    with pytest.raises(ValueError):
        parallel.SVMEval()                                           # n_classes is required
    ev = parallel.SVMEval(n_classes=3)
    with pytest.raises(ValueError, match="no training rows"):
        ev.fit()
    with pytest.raises(ValueError, match="fit"):
        ev.decision_function(X)
    with pytest.raises(ValueError, match="without a model"):
        ev.add_train(torch.zeros(2, 3, 8, 48, 48), torch.zeros(2, dtype=torch.int64))
