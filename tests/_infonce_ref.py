"""In-batch InfoNCE (avid_infonce, avid-cma_amd/csrc/infonce.hip): a float64 restatement, a float32 emulation in the
kernel's summation order, per-element error bounds derived from the kernel's structure, and the input makers.

Notation: S_ij = v_i . a_j / tau, lse_v[i] = logsumexp_j S_ij, lse_a[j] = logsumexp_i S_ij over the G keys of the global batch,
  L    = w_v mean_i (lse_v[i] - S_ii) + w_a mean_j (lse_a[j] - S_jj)
  W_ij = gs (w_v (exp(S_ij - lse_v[i]) - d_ij) + w_a (exp(S_ij - lse_a[j]) - d_ij)) / (tau G)
  dv_i = sum_j W_ij a_j,  da_j = sum_i W_ij v_i          for the local rows [row0, row0 + b).

The bounds (u = 2^-24, the unit roundoff of float32; the library's exp / log / expm1 are taken as good to 2 ulp = 4 u):
  score      one accumulator, D fused multiply-adds, then one product with float32(1 / tau):
             |dS| <= (D + 2) u |v||a| / tau                                                        (e_s; |v||a| <= 1.001)
  lse        lse = m + log(l) is exact for ANY shift m, so only l and the log count.  A term exp(s - m) carries the score
             error, the rounding of the difference (u 2 / tau), and exp's 4 u; 4 + 4 additions inside a tile (sequential, then
             a butterfly over 16 lanes); per key tile one rescale l * exp(m_old - m_new) + p: 3 roundings, exp's 4 u and the
             difference's u 2 / tau.  Relative errors of positive terms carry over to the sum; log turns them absolute.
             |dlse| <= e_s + u (2.01 / tau (1 + n_t) + 12 + 7 n_t + 5 ln G + 1 / tau)                 (e_lse; n_t = ceil(G / 64))
  loss       the row terms are added in double: (w_v + w_a) (e_lse + e_s) + 3 u |L|
  weight     p = exp(s - lse): relative error eps_p = e_s + e_lse + u (2.01 / tau + ln G) + 4 u; on the diagonal expm1 keeps
             the error of p - 1 at eps_p p + 4 u.  scale = gs / tau / G and the combination: 8 more roundings.
             |dW_ij| <= scale ((w_v p_v + w_a p_a)(eps_p + 8 u) + d_ij (w_v + w_a) 12 u)
  gradient   one accumulator per element, G fused multiply-adds in key order:
             |d dv_i[c]| <= sum_j |dW_ij| |a_j[c]| + 1.01 (G + 1) u sum_j |W_ij| |a_j[c]|
All first-order terms; SLACK covers the products of two of them."""
import numpy as np

U = 2.0 ** -24
SLACK = 1.05
KT = 64                      # keys of a tile (csrc/infonce.hip: IN_KT)


def _normalize64(x):
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def score_bound(D, inv_T):
    return SLACK * (D + 2) * U * 1.001 * inv_T


def _gap_ok(v, a, inv_T, factor=10.0):
    """Every row's and every column's top-two gap of S (float64) exceeds ``factor`` = ten times the score bound."""
    G, D = v.shape
    if G < 2:
        return True
    S = (v.astype(np.float64) @ a.astype(np.float64).T) * inv_T
    for M in (S, S.T):
        top = np.partition(M, -2, axis=1)[:, -2:]
        if float((top[:, 1] - top[:, 0]).min()) <= factor * score_bound(D, inv_T):
            return False
    return True


def _make(G, D, seed, inv_T, noise, factor=10.0):
    for attempt in range(200):
        rng = np.random.RandomState(seed + 7919 * attempt)
        v = _normalize64(rng.randn(G, D))
        a = _normalize64(rng.randn(G, D)) if noise is None else _normalize64(v + noise * rng.randn(G, D) / np.sqrt(D))
        v, a = v.astype(np.float32), a.astype(np.float32)
        if _gap_ok(v, a, inv_T, factor):
            return v, a
    raise AssertionError(f"no input with a top-two gap above 10 score bounds found for G={G}, D={D}, 1/T={inv_T}")


def make_unrelated(G, D, seed=0, inv_T=1.0 / 0.07):
    """Independent unit rows: a near-uniform softmax.  float32 [G, D] each."""
    return _make(G, D, seed, inv_T, None)


def make_trained(G, D, seed=0, inv_T=1.0 / 0.07, noise=0.3):
    """a_i = normalize(v_i + small noise): a peaked softmax in which p_ii - 1 cancels."""
    return _make(G, D, seed, inv_T, noise)


def extreme_small_tau():
    """tau = 0.005, unrelated rows: a fixed shift by 1 / tau underflows exp for every key of a row.  (v, a, 1 / tau)"""
    return make_unrelated(48, 128, 5, 200.0) + (200.0,)


def extreme_identical_pairs():
    """tau = 0.01, a_i == v_i: S_ii = 100, and exp(100) without a shift overflows float32.  (v, a, 1 / tau)"""
    v, _ = make_unrelated(48, 128, 6, 100.0)
    assert _gap_ok(v, v, 100.0)
    return v, v.copy(), 100.0


def ref64(v, a, inv_T, w=(0.5, 0.5), gs=1.0, row0=0, b=None):
    v64, a64 = np.asarray(v, np.float64), np.asarray(a, np.float64)
    G = v64.shape[0]
    b = G - row0 if b is None else b
    wv, wa = float(w[0]), float(w[1])
    S = (v64 @ a64.T) * inv_T

    def lse(M):
        m = M.max(axis=1, keepdims=True)
        return (m + np.log(np.exp(M - m).sum(axis=1, keepdims=True)))[:, 0]
    lse_v, lse_a = lse(S), lse(S.T)
    dg = np.diag(S)
    lv, la = float((lse_v - dg).mean()), float((lse_a - dg).mean())
    Pv, Pa = np.exp(S - lse_v[:, None]), np.exp(S - lse_a[None, :])
    I = np.eye(G)
    W = gs * (wv * (Pv - I) + wa * (Pa - I)) * inv_T / G
    ar = np.arange(G)
    return {"S": S, "lse_v": lse_v, "lse_a": lse_a, "loss": wv * lv + wa * la, "v2a": lv, "a2v": la,
            "hits": (int((S.argmax(axis=1) == ar).sum()), int((S.argmax(axis=0) == ar).sum())),
            "Pv": Pv, "Pa": Pa, "W": W, "dv": (W @ a64)[row0:row0 + b], "da": (W.T @ v64)[row0:row0 + b]}


def bounds(r, v, a, inv_T, w=(0.5, 0.5), gs=1.0, row0=0, b=None):
    """Per-quantity bounds for the float64 result ``r`` of ``ref64`` on the same arguments (see the module docstring)."""
    G, D = v.shape
    b = G - row0 if b is None else b
    wv, wa = float(w[0]), float(w[1])
    lnG, nt = np.log(G), -(-G // KT)
    e_s = score_bound(D, inv_T)
    e_lse = e_s + SLACK * U * (2.01 * inv_T * (1 + nt) + 12 + 7 * nt + 5 * lnG + inv_T)
    e_dir = SLACK * (e_lse + e_s)
    eps_p = e_s + e_lse + SLACK * U * (2.01 * inv_T + lnG + 4)
    scale = abs(gs) * inv_T / G
    EW = SLACK * scale * ((wv * r["Pv"] + wa * r["Pa"]) * (eps_p + 8 * U) + np.eye(G) * (wv + wa) * 12 * U)
    absW, av, aa = np.abs(r["W"]), np.abs(np.asarray(v, np.float64)), np.abs(np.asarray(a, np.float64))
    acc = SLACK * 1.01 * (G + 1) * U
    E_dv = (EW @ aa + acc * (absW @ aa))[row0:row0 + b]
    E_da = (EW.T @ av + acc * (absW.T @ av))[row0:row0 + b]
    return {"score": e_s, "lse": e_lse, "v2a": e_dir + 3 * U * abs(r["v2a"]), "a2v": e_dir + 3 * U * abs(r["a2v"]),
            "loss": (wv + wa) * e_dir + 3 * U * abs(r["loss"]), "dv": E_dv, "da": E_da}


DEFECTS = ("no_delta", "swap_lse", "no_key_role", "b_for_G", "tau_twice", "drop_tail", "fixed_shift", "no_shift")


def emulate32(v, a, inv_T, w=(0.5, 0.5), gs=1.0, row0=0, b=None, defect=None):
    """The kernel's arithmetic in float32 numpy, in its order: scores from one accumulator over d (a product and a sum per
    step where the kernel fuses them), the running-maximum softmax over key tiles of 64, the loss terms added in double,
    the gradient from one accumulator per element over the keys in index order.  ``defect``: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    f = np.float32
    v, a = np.asarray(v, f), np.asarray(a, f)
    G, D = v.shape
    b = G - row0 if b is None else b
    wv, wa, it = f(w[0]), f(w[1]), f(inv_T)
    with np.errstate(all="ignore"):
        acc = np.zeros((G, G), f)
        for d in range(D):
            acc = acc + v[:, d:d + 1] * a[None, :, d]
        S = acc * it
        if defect == "tau_twice":
            S = S * it
        Gk = G - G % KT if defect == "drop_tail" and G % KT and G > KT else G

        def lse_hits(M):
            m = np.full(G, -np.inf, f)
            l = np.zeros(G, f)
            am = np.zeros(G, np.int64)
            for k0 in range(0, Gk, KT):
                t = M[:, k0:min(k0 + KT, Gk)]
                tm, ti = t.max(axis=1), t.argmax(axis=1) + k0
                am = np.where(tm > m, ti, am)
                mn = np.maximum(m, tm)
                if defect == "fixed_shift":
                    mn = np.full(G, it, f)
                elif defect == "no_shift":
                    mn = np.zeros(G, f)
                p = np.zeros(G, f)
                for c in range(t.shape[1]):
                    p = p + np.exp(t[:, c] - mn)
                l = l * np.exp(m - mn) + p if defect not in ("fixed_shift", "no_shift") else l + p
                m = mn
            return (m + np.log(l)).astype(f), am
        lse_v, am_v = lse_hits(S)
        lse_a, am_a = lse_hits(np.ascontiguousarray(S.T))
        dg = np.diag(S).astype(np.float64)
        lv, la = float((lse_v.astype(np.float64) - dg).sum() / G), float((lse_a.astype(np.float64) - dg).sum() / G)
        scale = f(f(gs) * it) / f(b if defect == "b_for_G" else G)
        I = np.eye(G, dtype=bool)

        def weights(own, oth, M, w_own, w_oth):          # rows: the queries; M[q][k]
            if defect == "swap_lse":
                own, oth = oth, own
            x_own, x_oth = M - own[:, None], M - oth[None, :]
            if defect == "no_delta":
                t_own, t_oth = np.exp(x_own), np.exp(x_oth)
            else:
                t_own = np.where(I, np.expm1(x_own), np.exp(x_own)).astype(f)
                t_oth = np.where(I, np.expm1(x_oth), np.exp(x_oth)).astype(f)
            if defect == "no_key_role":
                t_oth = np.zeros_like(t_oth)
            return (scale * (w_own * t_own + w_oth * t_oth)).astype(f)
        Wv = weights(lse_v, lse_a, S, wv, wa)[row0:row0 + b]
        Wa = weights(lse_a, lse_v, np.ascontiguousarray(S.T), wa, wv)[row0:row0 + b]
        dv, da = np.zeros((b, D), f), np.zeros((b, D), f)
        for c in range(Gk):
            dv = dv + Wv[:, c:c + 1] * a[c][None, :]
            da = da + Wa[:, c:c + 1] * v[c][None, :]
    ar = np.arange(G)
    return {"S": S, "lse_v": lse_v, "lse_a": lse_a, "loss": float(f(float(wv) * lv + float(wa) * la)), "v2a": float(f(lv)),
            "a2v": float(f(la)), "hits": (int((am_v == ar).sum()), int((am_a == ar).sum())), "dv": dv, "da": da}


def excess(got, r, bd):
    """The worst ratio |got - reference| / bound over loss, direction losses and gradient elements (inf if non-finite)."""
    worst = 0.0
    for k in ("loss", "v2a", "a2v", "dv", "da"):
        g = np.asarray(got[k], np.float64)
        if not np.all(np.isfinite(g)):
            return float("inf")
        worst = max(worst, float((np.abs(g - r[k]) / np.maximum(bd[k], 1e-300)).max()))
    return worst
