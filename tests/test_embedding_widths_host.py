"""CPU-only acceptance of tests/_width_ref.py: the error bounds the GPU tests (tests/test_gpu_embedding_widths.py) hold the
criterion kernels to are

* SAFE: the same operation in float32 with torch on the CPU stays inside them at every shape the GPU tests use, and
* SHARP: each wrong-width mutation of the float64 restatement (a dropped 64-float slice, two slices swapped, a row pitch left
  at 128, the neighbouring row, a dropped last row, the wrong duplicate, the EMA of an already updated row) puts at least one
  element 10 x outside them, at those same inputs;

the correspondence-search banks have tie-free top-(k + 1) lists wherever the GPU test asks for equal sets; and the float32
oracle's own deviation from the float64 oracle is a quarter or less of every tolerance the criterion-step test uses.
"""
import numpy as np
import pytest
import torch

import _width_ref as W

FACTOR = 10.0


def worst(got, want, bound):
    """max over elements of |got - want| / bound (an element with bound 0 must be equal: inf otherwise)."""
    diff = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / bound)
    return float(r.max())


def pitched(a, pitch=128):
    """Row r read at element offset r * pitch of the flattened array instead of r * D (wrapping at the end)."""
    a = np.asarray(a, np.float64)
    n, D = a.shape
    flat = a.reshape(-1)
    return flat[(np.arange(n)[:, None] * pitch + np.arange(D)[None]) % flat.size]


def swap01(a):
    """The first two 64-wide slices of the last axis exchanged."""
    a = np.array(a, np.float64)
    a[..., :64], a[..., 64:128] = a[..., 64:128].copy(), a[..., :64].copy()
    return a


# ---- F.normalize ------------------------------------------------------------------------------------------------------------
L2_CASES = [(bs, D) for D in W.L2_WIDTHS for bs in W.L2_BS]


@pytest.mark.parametrize("bs,D", L2_CASES)
def test_normalize_bounds_hold_in_float32(bs, D):
    x, dy = W.l2_inputs(bs, D)
    n = (x * x).sum(1).sqrt().clamp_min(1e-12)
    y = x / n[:, None]
    dx = (dy - y * (y * dy).sum(1, keepdim=True)) * (1.0 / n)[:, None]
    want, _ = W.normalize_fwd(x)
    r_f, r_b = worst(y.numpy(), want, W.normalize_fwd_bound(x)), worst(dx.numpy(), W.normalize_bwd(x, dy), W.normalize_bwd_bound(x, dy))
    print(f"l2 bs {bs} D {D}: float32 forward at {r_f:.3f} of its bound, backward at {r_b:.3f}")
    assert r_f <= 1 and r_b <= 1
    if bs > W.L2_ZERO_ROW:
        assert (want[W.L2_ZERO_ROW] == 0).all() and (W.normalize_fwd_bound(x)[W.L2_ZERO_ROW] == 0).all()


def _l2_mutations(bs, D):
    """name -> (mutated forward, mutated backward)"""
    x, dy = (W._f64(t) for t in W.l2_inputs(bs, D))
    cut = W.last_slice(D)
    out = {}
    xs = x.copy()
    xs[:, cut:] = 0                                       # the last trip of the sum of squares / of <y, dy> never ran
    n = np.maximum(np.sqrt((xs * xs).sum(1)), 1e-12)
    y, nt = W.normalize_fwd(x)
    dot = (y[:, :cut] * dy[:, :cut]).sum(1)
    out["last slice dropped"] = (x / n[:, None], (dy - y * dot[:, None]) / nt[:, None])
    if D >= 128:
        out["slices swapped"] = (swap01(y), swap01(W.normalize_bwd(x, dy)))
    if bs > 1 and D != 128:
        xp = pitched(x)
        out["pitch 128"] = (W.normalize_fwd(xp)[0], W.normalize_bwd(xp, dy))
    if bs > 1:
        f, b = y.copy(), W.normalize_bwd(x, dy)
        f[bs - 1], b[bs - 1] = 0, 0
        out["last row dropped"] = (f, b)
    return out


@pytest.mark.parametrize("bs,D", L2_CASES)
def test_normalize_bounds_catch_the_mutations(bs, D):
    x, dy = W.l2_inputs(bs, D)
    want_f, want_b = W.normalize_fwd(x)[0], W.normalize_bwd(x, dy)
    bf, bb = W.normalize_fwd_bound(x), W.normalize_bwd_bound(x, dy)
    keep = np.arange(bs) != W.L2_ZERO_ROW if bs > W.L2_ZERO_ROW else np.ones(bs, bool)     # the backward's masked row
    for name, (f, b) in _l2_mutations(bs, D).items():
        r_f, r_b = worst(f, want_f, bf), worst(b[keep], want_b[keep], bb[keep])
        print(f"l2 bs {bs} D {D} {name}: forward {r_f:.3g} x bound, backward {r_b:.3g} x bound")
        assert r_f >= FACTOR, (name, r_f)
        if D > 1:                      # (D = 1: y = +-1 and dx = dy (1 - y^2) / norm is 0 whatever the row: only the forward can tell)
            assert r_b >= FACTOR, (name, r_b)


# ---- scores and their gradient ---------------------------------------------------------------------------------------------
SCORE_CASES = [(D, bs, R) for D in W.SCORE_WIDTHS for bs, R in W.SCORE_SHAPES] + \
              [(D, 3, R) for D in W.ABI_WIDTHS for R in W.ABI_R if (3, R) not in W.SCORE_SHAPES]


@pytest.mark.parametrize("D,bs,R", SCORE_CASES)
def test_score_bounds_hold_in_float32(D, bs, R):
    bank, emb, idx, ds = W.score_inputs(D, bs, R)
    inv_T = torch.tensor(W.INV_T, dtype=torch.float32)
    s = (bank[idx] * emb[:, None, :]).sum(-1) * inv_T
    g = (ds[:, :, None] * bank[idx]).sum(1) * inv_T
    r_s = worst(s.numpy(), W.scores(bank, emb, idx), W.scores_bound(bank, emb, idx))
    r_g = worst(g.numpy(), W.scores_grad(bank, idx, ds), W.scores_grad_bound(bank, idx, ds))
    print(f"scores D {D} bs {bs} R {R}: float32 scores at {r_s:.3f} of their bound, d emb at {r_g:.3f}")
    assert r_s <= 1 and r_g <= 1
    # the inputs are what the GPU test says they are
    want = W.scores(bank, emb, idx)
    assert np.allclose(want[:, R - 1], W.INV_T, rtol=1e-6)                 # the planted positive: 1/T
    assert int(idx.max()) == W.SCORE_N - 1 and (R == 1 or int(idx.min()) == 0)


def _score_mutations(D, bs, R):
    """name -> (mutated scores, mutated d emb)"""
    bank, emb, idx, ds = W.score_inputs(D, bs, R)
    bank, emb, ds, idx = W._f64(bank), W._f64(emb), W._f64(ds), idx.numpy()
    cut = D - 64
    out = {}
    g = W.scores_grad(bank, idx, ds)
    g[:, cut:] = 0
    out["last slice dropped"] = (W.scores(bank[:, :cut], emb[:, :cut], idx), g)
    if D >= 128:
        out["slices swapped"] = (W.scores(bank, swap01(emb), idx), swap01(W.scores_grad(bank, idx, ds)))
    if D != 128:
        bp = pitched(bank)
        out["pitch 128"] = (W.scores(bp, emb, idx), W.scores_grad(bp, idx, ds))
    if R > 1:
        nxt = np.roll(idx, -1, axis=1)
        out["row j + 1"] = (W.scores(bank, emb, nxt), W.scores_grad(bank, nxt, ds))
    s, d2 = W.scores(bank, emb, idx), ds.copy()
    s[:, R - 1], d2[:, R - 1] = 0, 0
    out["last row dropped"] = (s, W.scores_grad(bank, idx, d2))
    return out


@pytest.mark.parametrize("D,bs,R", SCORE_CASES)
def test_score_bounds_catch_the_mutations(D, bs, R):
    bank, emb, idx, ds = W.score_inputs(D, bs, R)
    want_s, want_g = W.scores(bank, emb, idx), W.scores_grad(bank, idx, ds)
    b_s, b_g = W.scores_bound(bank, emb, idx), W.scores_grad_bound(bank, idx, ds)
    for name, (s, g) in _score_mutations(D, bs, R).items():
        r_s, r_g = worst(s, want_s, b_s), worst(g, want_g, b_g)
        print(f"scores D {D} bs {bs} R {R} {name}: scores {r_s:.3g} x bound, d emb {r_g:.3g} x bound")
        assert r_s >= FACTOR, (name, r_s)
        assert r_g >= FACTOR, (name, r_g)


# ---- EMA + renormalise ------------------------------------------------------------------------------------------------------
UPDATE_CASES = [(D, B, m) for D in W.UPDATE_WIDTHS for B in W.UPDATE_B for m in W.MOMENTA]


@pytest.mark.parametrize("D,B,m", UPDATE_CASES)
def test_update_bound_holds_in_float32(D, B, m):
    bank, emb, _, y = W.update_inputs(D, B)
    got = bank.clone()
    m32 = torch.tensor(m, dtype=torch.float32)
    for i in range(B):                                             # sequential from the OLD rows: the last duplicate wins
        t = bank[y[i]] * m32 + emb[i] * (1 - m32)
        got[y[i]] = t / (t * t).sum().sqrt().clamp_min(1e-12)
    want, bound = W.bank_update(bank, y, emb, m)
    r = worst(got.numpy(), want, bound)
    print(f"update D {D} B {B} m {m}: float32 at {r:.3f} of the bound")
    assert r <= 1
    untouched = np.setdiff1d(np.arange(W.UPDATE_N), y.numpy())
    assert (bound[untouched] == 0).all() and (bound[y.numpy()] > 0).any()
    if B >= 5:
        a, b, c = W.update_duplicates(B)
        assert y[a] == y[b] == y[c] and c < B - 1 and (y == 0).any() and (y == W.UPDATE_N - 1).any()
        assert len(set(y.tolist())) == B - 2                       # no other duplicates


def _update_mutations(D, B, m):
    bank, emb, _, y = W.update_inputs(D, B)
    bank, emb, y = W._f64(bank), W._f64(emb), y.numpy()
    want, _ = W.bank_update(bank, y, emb, m)
    cut = W.last_slice(D)
    owned = np.unique(y)
    out = {}
    a = bank.copy()
    part, _ = W.bank_update(bank[:, :cut], y, emb[:, :cut], m) if cut else (bank[:, :0], None)
    a[:, :cut] = part                                              # the last trip never ran: not summed, not written
    out["last slice dropped"] = a
    if D >= 128:
        a = want.copy()
        a[owned] = swap01(want[owned])
        out["slices swapped"] = a
    if D != 128:
        flat = bank.copy().reshape(-1)                             # rows written at pitch 128
        for r in owned:
            flat[(r * 128 + np.arange(D)) % flat.size] = want[r]
        out["pitch 128"] = flat.reshape(bank.shape)
    if B > 1:
        out["row i + 1"] = W.bank_update(bank, y, np.roll(emb, -1, axis=0), m)[0]
    out["last row dropped"] = W.bank_update(bank, y[:B - 1], emb[:B - 1], m)[0]
    if B >= 5:
        out["first duplicate wins"] = W.bank_update(bank, y[::-1], emb[::-1], m)[0]
        a = bank.copy()
        for i in range(B):                                         # every sample applied to the row as it finds it
            a = W.bank_update(a, y[i:i + 1], emb[i:i + 1], m)[0]
        out["EMA of the updated row"] = a
    return out


@pytest.mark.parametrize("D,B,m", UPDATE_CASES)
def test_update_bound_catches_the_mutations(D, B, m):
    bank, emb, _, y = W.update_inputs(D, B)
    want, bound = W.bank_update(bank, y, emb, m)
    for name, got in _update_mutations(D, B, m).items():
        r = worst(got, want, bound)
        print(f"update D {D} B {B} m {m} {name}: {r:.3g} x bound")
        assert r >= FACTOR, (name, r)


# ---- the correspondence-search banks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(N, D) for D in W.TOPK_WIDTHS for N in W.TOPK_N])
def test_topk_banks_are_free_of_ties(N, D):
    """The oracle's own float32 search passes what the GPU test asks of the kernels (W.topk_check: containment within the
    float32 tolerance of the float64 scores) and differs from the float64 top-k in fewer than 0.1 % of the queries, never by
    more than one row: half of what the comparison rule of test_cma_topk_filter_path_vs_oracle allows (> 99.8 % equal sets,
    >= k - 1 common rows), so that rule is one the banks let a correct float32 search meet."""
    from oracle import avid_oracle as O
    v1, v2 = W.topk_banks(N, D)
    got = {kind: O.cma_topk(v1, v2, W.TOPK_K, kind) for kind in W.TOPK_KINDS}
    for kind, (same, common) in W.topk_check(N, D, got).items():
        print(f"N {N} D {D} {kind}: float32 oracle finds the float64 set for {same:.4%} of the queries, >= {common} rows in common")
        assert same > 0.999 and common >= W.TOPK_K - 1


# ---- criterion steps: the float32 oracle against the float64 oracle ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["avid", "cma"])
@pytest.mark.parametrize("D", W.CRIT_WIDTHS)
def test_float32_oracle_deviation_is_a_quarter_of_the_tolerances(kind, D):
    """The GPU test compares with the float64 oracle at the project's tolerances (W.CRIT_TOL); the reference those were set
    against is float32, so they must leave the kernel the reference's own noise plus a margin: the float32 oracle may use up
    at most a quarter of each.  (Figures in the docstring of test_gpu_embedding_widths.test_criterion_two_steps.)"""
    lo, hi = W.oracle_steps(kind, D, torch.float32), W.oracle_steps(kind, D, torch.float64)
    for step, (a, b) in enumerate(zip(lo, hi)):
        dev = {"loss": W.deviation(a["loss"], b["loss"], W.CRIT_TOL["loss"]), "Z": W.deviation(a["Z"], b["Z"], W.CRIT_TOL["Z"]),
               "tb": max(W.deviation(a["tb"][k], b["tb"][k], W.CRIT_TOL["tb"]) for k in b["tb"]),
               "grad": max(W.deviation(a[k], b[k], W.CRIT_TOL["grad"]) for k in ("gv", "ga")),
               "rows": max(W.deviation(a[k], b[k], W.CRIT_TOL["rows"]) for k in ("v1rows", "v2rows"))}
        print(f"{kind} D {D} step {step}: float32 oracle uses " + ", ".join(f"{k} {v:.3f}" for k, v in dev.items()) + " of the tolerance")
        assert set(a["tb"]) == set(b["tb"]) and len(b["tb"]) >= 4
        for k, v in dev.items():
            assert v <= 0.25, (kind, D, step, k, v)
    assert lo[1]["Z"] == lo[0]["Z"] and hi[1]["Z"] == hi[0]["Z"]          # Z is frozen after the first step
