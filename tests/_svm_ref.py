"""float64 restatement of the linear one-vs-all SVM (csrc/svm.hip, ops.svm_fit) for tests/test_svm_host.py and
tests/test_gpu_svm.py: objective, gradient and generalised Hessian of liblinear's L2-regularised L2-loss primal, a Newton
solver run to |grad f| <= 1e-10 |grad f(0)|, the two products, float32 restatements of the kernels' summation structure and
the per-element error bounds derived from that structure.

The problem, per class c (y = +1 where label == c, else -1; x~ = (x, s), s = intercept_scaling; wa = (w, beta)):

    f_c(wa) = 0.5 |wa|^2 + sum_i cost_ic max(0, 1 - y_i wa . x~_i)^2,     cost_ic = cost * (pos_weight[c] if y_i > 0 else 1)

f_c is 1-strongly convex: |wa - wa*| <= |grad f_c(wa)| for every wa (and <= |g| + |g*| against a point wa* with gradient g*).

Bounds.  u = 2^-24.  A chain of n float32 fused multiply-adds started from zero, s = fma(a_n, b_n, ... fma(a_1, b_1, 0)), carries
n roundings, and every further float32 operation its value passes through one more: |s - sum a b| <= gamma_n sum |a||b| with
gamma_n = n u / (1 - n u), n the roundings on the longest path (Higham, Accuracy and Stability, 3.1 / 3.4).

* scores: element = (s0 + s1) + bias; s0 is the chain over the features f % 4 in {0, 1}, s1 over f % 4 in {2, 3}, ascending.
  The longest chain has chain_len(F) = 2 (F // 4) + min(F % 4, 2) terms, then two additions: n = chain_len(F) + 2.
  (Zero padding adds fma(0, 0, acc) = acc: no rounding.)
* xt: a slice of SLICE rows gives the partial (s0 + s1), chains over the row index % 4: chain_len(rows) + 1 roundings; the
  partials are added in double (below 2^-53 per addition: one more u covers any slice count that fits memory) and rounded to
  float32 once: n = chain_len(min(N, SLICE)) + 3.
* column sums: double accumulation, one rounding: n = 2 (the second u covers the double additions).
"""
import numpy as np

U = 2.0 ** -24
SLICE = 512            # rows per slice of avid_svm_xt (ops.SVM_SLICE_ROWS)


def gamma(n):
    return n * U / (1.0 - n * U)


def chain_len(n):
    return 2 * (n // 4) + min(n % 4, 2)


# ---- the problem -----------------------------------------------------------------------------------------------------------
def targets(labels, C):
    return np.where(np.asarray(labels)[:, None] == np.arange(C)[None, :], 1.0, -1.0)


def costs(labels, C, cost=1.0, pos_weight=None):
    pw = np.ones(C) if pos_weight is None else np.asarray(pos_weight, np.float64)
    return np.where(targets(labels, C) > 0, float(cost) * pw[None, :], float(cost))


def augmented(X, s=1.0):
    X = np.asarray(X, np.float64)
    return np.concatenate([X, np.full((X.shape[0], 1), float(s))], 1)


def objective(Wa, Xa, Y, Cst):
    """f_c for every class: Wa [C, F + 1], Xa [N, F + 1], Y / Cst [N, C] -> [C]."""
    m = np.maximum(1.0 - Y * (Xa @ Wa.T), 0.0)
    return 0.5 * (Wa * Wa).sum(1) + (Cst * m * m).sum(0)


def gradient(Wa, Xa, Y, Cst):
    m = np.maximum(1.0 - Y * (Xa @ Wa.T), 0.0)
    return Wa - 2.0 * (Cst * Y * m).T @ Xa


def hessian(wa, Xa, y, cst):
    """The generalised Hessian of one class: I + 2 X~^T diag(cost * active) X~."""
    act = (1.0 - y * (Xa @ wa) > 0).astype(np.float64) * cst
    return np.eye(Xa.shape[1]) + 2.0 * (Xa * act[:, None]).T @ Xa


def newton_solve(X, labels, C, cost=1.0, pos_weight=None, s=1.0, rel=1e-10, max_iter=200):
    """(Wa [C, F + 1], iterations [C], converged [C]): exact Newton steps with a backtracking search per class, stopped at
    |grad| <= rel |grad(0)|."""
    Xa, Y, Cst = augmented(X, s), targets(labels, C), costs(labels, C, cost, pos_weight)
    Wa = np.zeros((C, Xa.shape[1]))
    iters, conv = np.zeros(C, np.int64), np.zeros(C, bool)
    for c in range(C):
        y, cst, wa = Y[:, c:c + 1], Cst[:, c:c + 1], np.zeros(Xa.shape[1])
        g0 = np.linalg.norm(gradient(wa[None], Xa, y, cst)[0])
        for it in range(max_iter + 1):
            g = gradient(wa[None], Xa, y, cst)[0]
            if np.linalg.norm(g) <= rel * g0:
                conv[c] = True
                break
            if it == max_iter:
                break
            d = -np.linalg.solve(hessian(wa, Xa, y[:, 0], cst[:, 0]), g)
            f, t = objective(wa[None], Xa, y, cst)[0], 1.0
            while objective((wa + t * d)[None], Xa, y, cst)[0] > f + 1e-4 * t * (g @ d) and t > 1e-12:
                t *= 0.5
            wa = wa + t * d
            iters[c] = it + 1
        Wa[c] = wa
    return Wa, iters, conv


# ---- the two products ------------------------------------------------------------------------------------------------------
def scores64(X, W, b=None):
    z = np.asarray(X, np.float64) @ np.asarray(W, np.float64).T
    return z if b is None else z + np.asarray(b, np.float64)[None, :]


def xt64(X, D):
    D = np.asarray(D, np.float64)
    return D.T @ np.asarray(X, np.float64), D.sum(0)


def scores_bound(X, W, b=None, extra=0):
    """Per-element bound of avid_svm_scores against scores64 (``extra``: further roundings on the way, e.g. of the bias)."""
    F = np.asarray(X).shape[1]
    mag = np.abs(np.asarray(X, np.float64)) @ np.abs(np.asarray(W, np.float64)).T
    if b is not None:
        mag = mag + np.abs(np.asarray(b, np.float64))[None, :]
    return gamma(chain_len(F) + 2 + extra) * mag


def xt_bound(X, D):
    """(bound of g [C, F], bound of gb [C]) of avid_svm_xt against xt64."""
    N = np.asarray(X).shape[0]
    absD = np.abs(np.asarray(D, np.float64))
    return gamma(chain_len(min(N, SLICE)) + 3) * (absD.T @ np.abs(np.asarray(X, np.float64))), gamma(2) * absD.sum(0)


def _fma32(a, b, c):
    # a * b is exact in double (24 + 24 bits); the sum is rounded to double, then to float32
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _chains32(A, B):
    """(s0 + s1) of the kernels for out[m][n] = sum_k A[k][m] B[k][n] in float32: the chain over k % 4 in {0, 1} plus the
    chain over k % 4 in {2, 3}, each in ascending k."""
    s = [np.zeros((A.shape[1], B.shape[1]), np.float32) for _ in range(2)]
    for k in range(A.shape[0]):
        j = (k % 4) // 2
        s[j] = _fma32(A[k][:, None], B[k][None, :], s[j])
    return s[0] + s[1]


def scores_f32(X, W, b=None, fault=None):
    """avid_svm_scores restated in float32.  ``fault``: "remainder" drops the last F % 4 features, "bias" omits the bias,
    "pitch" places class block b of W at row 63 b instead of 64 b (a block read at the wrong pitch)."""
    X, W = np.asarray(X, np.float32), np.asarray(W, np.float32)
    F = X.shape[1]
    if fault == "remainder":
        F -= F % 4
    if fault == "pitch":
        W = np.stack([W[c - c // 64] for c in range(W.shape[0])])
    z = _chains32(X[:, :F].T, W[:, :F].T)
    if b is not None and fault != "bias":
        z = z + np.asarray(b, np.float32)[None, :]
    return z


def xt_f32(X, D, fault=None):
    """avid_svm_xt restated in float32: (g, gb).  ``fault``: "slice" drops the last slice of rows."""
    X, D = np.asarray(X, np.float32), np.asarray(D, np.float32)
    N = X.shape[0]
    nsl = -(-N // SLICE)
    if fault == "slice":
        nsl -= 1
    g, gb = np.zeros((D.shape[1], X.shape[1])), np.zeros(D.shape[1])
    for k in range(nsl):
        rows = slice(k * SLICE, min(N, (k + 1) * SLICE))
        g += _chains32(D[rows], X[rows]).astype(np.float64)
        gb += D[rows].astype(np.float64).sum(0)
    return g.astype(np.float32), gb.astype(np.float32)


# ---- bounds of what the solver evaluates in float32 ----------------------------------------------------------------------------
def _eval_terms(coef, intercept, X, labels, cost, pos_weight, s):
    """At the float32 iterate (coef, intercept = s beta): Xa, Wa, Y, Cst, the margins' positive parts in float64 and the bound
    Ez of the kernels' scores (the bias s * beta carries one more rounding when s is not a power of two)."""
    C = np.asarray(coef).shape[0]
    Xa, Y, Cst = augmented(X, s), targets(labels, C), costs(labels, C, cost, pos_weight)
    Wa = np.concatenate([np.asarray(coef, np.float64), np.asarray(intercept, np.float64)[:, None] / float(s)], 1)
    mp = np.maximum(1.0 - Y * (Xa @ Wa.T), 0.0)
    Ez = scores_bound(X, coef, intercept, extra=1)
    return Xa, Wa, Y, Cst, mp, Ez


def gradient_eval_bound(coef, intercept, X, labels, cost=1.0, pos_weight=None, s=1.0):
    """E_c [C]: the 2-norm of the per-element bound of the float32 gradient the solver evaluates (scores -> hinge residual ->
    xt -> w - 2 G) against ``gradient`` at the same iterate.
      z:  |dz| <= Ez.
      r = (y m) cost_ic, m = fma(-y, z, 1), cost_ic = fl(cost pos_weight): max(0, .) is 1-Lipschitz, three roundings:
          |dr| <= cost_ic (Ez + 4u (m+ + Ez)),  |r^| <= cost_ic (m+ + Ez) =: R.
      G = xt(r^): |dG| <= xt_bound(X~, R) + |X~|^T |dr| (the intercept column: double column sums times s, inside the same
          gamma), one more rounding for gb * s.
      g = fl(w - 2 G): |dg| <= 2 |dG| + u (|w| + 2 (|G| + |dG|))."""
    Xa, Wa, Y, Cst, mp, Ez = _eval_terms(coef, intercept, X, labels, cost, pos_weight, s)
    dr = Cst * (Ez + 4 * U * (mp + Ez))
    R = Cst * (mp + Ez)
    absXa = np.abs(Xa)
    dG = xt_bound(Xa, R)[0] + dr.T @ absXa + U * (R.T @ absXa)
    G = np.abs((Cst * Y * mp).T @ Xa)
    dg = 2.0 * dG + U * (np.abs(Wa) + 2.0 * (G + dG))
    return np.sqrt((dg * dg).sum(1))


def objective_eval_bound(coef, intercept, X, labels, cost=1.0, pos_weight=None, s=1.0):
    """[C]: bound of info["objective"] (0.5 |wa|^2 in double plus avid_svm_loss: double sums over the float32 scores) against
    ``objective`` at the same iterate: |m^+^2 - m+^2| <= Ez (2 m+ + Ez) per row, the cost's rounding, double round-off."""
    Xa, Wa, Y, Cst, mp, Ez = _eval_terms(coef, intercept, X, labels, cost, pos_weight, s)
    f = objective(Wa, Xa, Y, Cst)
    return (Cst * Ez * (2.0 * mp + Ez)).sum(0) + 2 * U * (Cst * mp * mp).sum(0) + 1e-12 * f


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def lattice(rng, shape, lo, hi, den):
    """Integers lo..hi over den: products and sums of such values are exact in float32 at the tests' sizes."""
    return (rng.integers(lo, hi + 1, size=shape) / float(den)).astype(np.float32)


def blobs(N, F, C, seed, absent=None, spread=1.0, sep=0.8):
    """Overlapping Gaussian blobs (class means sep apart per unit spread, so the active set is mixed at the optimum):
    (X float32 [N, F], labels int64 [N]); ``absent``: a class that gets no row."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((C, F)) * sep / np.sqrt(F)
    present = [c for c in range(C) if c != absent]
    labels = np.array([present[i % len(present)] for i in range(N)], np.int64)
    rng.shuffle(labels)
    X = means[labels] + spread * rng.standard_normal((N, F)) / np.sqrt(F)
    return X.astype(np.float32), labels


SOLVER_CASES = {      # name: (N, F, C, absent class, cost, pos_weight of class 1, intercept_scaling)
    "n193_f33_c3": (193, 33, 3, None, 1.0, None, 2.0),
    "n600_f64_c65": (600, 64, 65, None, 0.5, 2.0, 1.0),
    "n400_f40_c5_absent": (400, 40, 5, 3, 1.0, None, 1.0),
}


def solver_case(name):
    """(X, labels, C, cost, pos_weight float32 [C] or None, s) of a solver test, and held-out rows of the same blobs."""
    N, F, C, absent, cost, pw1, s = SOLVER_CASES[name]
    X, labels = blobs(N + 64, F, C, seed=sum(map(ord, name)), absent=absent)
    pw = None
    if pw1 is not None:
        pw = np.ones(C, np.float32)
        pw[1] = pw1
    return dict(X=X[:N], labels=labels[:N], C=C, cost=cost, pos_weight=pw, s=s, X_test=X[N:], labels_test=labels[N:])
