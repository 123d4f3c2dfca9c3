"""float64 restatements of the criterion ops whose code depends on the embedding width D (``avid_l2norm_*``,
``avid_bank_scores_*``, ``avid_bank_update*``), the per-element forward-error bounds the HIP kernels are held to, and the
inputs that tests/test_embedding_widths_host.py (CPU) and tests/test_gpu_embedding_widths.py (GPU) share.  numpy / torch on
the CPU; nothing here is shared with the code under test.

The bounds have the form c * u * S: u = 2^-24 (float32 unit roundoff), S the sum of the absolute values of the terms an
element adds up (from the float64 reference) and c the number of roundings on the longest path through the kernel, counted
from csrc/criterion.hip next to each bound.  They are first-order bounds (terms in u^2 dropped: < 1e-5 of the bound).  A
fraction of the output's largest value is the wrong yardstick: for random unit vectors the scores shrink like 1/sqrt(D)
while the rounding error does not.

The host test shows every bound (a) holding against the same arithmetic in float32 on the CPU and (b) caught by a factor
>= 10 by each wrong-width mutation of the float64 restatement (a dropped 64-float slice, a row pitch left at 128, ...).
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
INV_T = float(np.float32(1.0 / 0.07))          # the kernels take 1/T as a float: the reference uses that value

# ---- the shapes: the smallest at which each code path still exists ----------------------------------------------------------
L2_WIDTHS = (1, 63, 64, 65, 129, 256, 512, 1000)       # under / exactly / past one 64-lane trip, many trips, a ragged last trip
L2_BS = (1, 5)                                         # 5 rows: ragged against 4 rows per block
L2_ZERO_ROW = 3                                        # at bs = 5: the clamped zero row
SCORE_WIDTHS = (64, 128, 256, 512)                     # the four template instances (128: the control)
SCORE_SHAPES = ((1, 1), (3, 17), (3, 65), (2, 1025))   # one row, a ragged wave of 16, one row past a 64-row block, several blocks
SCORE_N = 300
ABI_WIDTHS = (64, 128, 512)
ABI_R = (17, 300)
UPDATE_WIDTHS = (64, 100, 256, 448, 512)               # 100: ragged last trip; 448 / 512: the last two register slots
UPDATE_B = (1, 5, 40)
UPDATE_N = 97
MOMENTA = (0.5, 0.9)


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def trips(D):
    """Trips of a wave's ``for (d = lane; d < D; d += 64)`` loop."""
    return -(-D // 64)


def last_slice(D):
    """First element of the last (possibly partial) 64-wide slice of a row."""
    return 64 * (trips(D) - 1)


# ---- F.normalize(x, p=2, dim=1) ---------------------------------------------------------------------------------------------
def normalize_fwd(x):
    """(y, norm): y = x / max(|x|, 1e-12) per row."""
    x = _f64(x)
    n = np.maximum(np.sqrt((x * x).sum(1)), 1e-12)
    return x / n[:, None], n


def normalize_fwd_bound(x):
    """Relative: every term of the sum of squares is positive.  l2norm_fwd_kernel: per lane trips(D) products and adds
    (fused or not: <= trips + 1 roundings on ss), 6 wave-reduction adds, halved by the square root, + the square root's own
    rounding + the division's: (trips + 7) / 2 + 2 <= trips + 5 roundings.  A zero row gives 0 * anything: bound 0."""
    y, _ = normalize_fwd(x)
    return (trips(y.shape[1]) + 5) * U * np.abs(y)


def normalize_bwd(x, dy):
    """dx = (dy - y <y, dy>) / norm with y, norm from the float64 forward."""
    y, n = normalize_fwd(x)
    dy = _f64(dy)
    dot = (y * dy).sum(1)
    return (dy - y * dot[:, None]) / n[:, None]


def normalize_bwd_bound(x, dy):
    """Absolute (dy - y <y, dy> cancels): c * u * S_d with S_d = (|dy_d| + |y_d| * sum_k |y_k dy_k|) / norm, t = trips(D).
    l2norm_bwd_kernel reads the forward's float32 y (relative error <= (t + 5) u, above) and norm (<= (t + 5) u):
      the dot product: (t + 5) u from y, + 1 product, t adds, 6 wave adds            -> (2t + 12) u * sum|y dy|, times |y_d|
      y_d * dot: y's error (t + 5) + the product's rounding                           -> (t + 6) u * |y_d dot|
      the subtraction, 1 / norm (norm's error t + 5, + the reciprocal's rounding), the final product -> (t + 8) u * |dy_d - y_d dot|
    each of the three <= its count * u * S_d: c = 4t + 26."""
    y, n = normalize_fwd(x)
    dy = _f64(dy)
    A = np.abs(y * dy).sum(1)
    S = (np.abs(dy) + np.abs(y) * A[:, None]) / n[:, None]
    return (4 * trips(y.shape[1]) + 26) * U * S


# ---- scores[b][j] = <bank[idx[b][j]], emb[b]> / T and d scores / d emb ------------------------------------------------------
def scores(bank, emb, idx, inv_T=INV_T):
    rows = _f64(bank)[np.asarray(idx)]
    return np.einsum("brd,bd->br", rows, _f64(emb)) * inv_T


def scores_bound(bank, emb, idx, inv_T=INV_T):
    """bank_scores_fwd_kernel<DPL>, D = 64 DPL: per lane DPL products and DPL adds, a 6-step wave reduction, the product
    with 1/T: c = 2 D / 64 + 7.  S = (1/T) sum_d |bank[r][d] emb[b][d]|."""
    rows = _f64(bank)[np.asarray(idx)]
    S = np.einsum("brd,bd->br", np.abs(rows), np.abs(_f64(emb))) * inv_T
    return (2 * (rows.shape[2] // 64) + 7) * U * S


def scores_grad(bank, idx, ds, inv_T=INV_T):
    """demb[b][d] = (1/T) sum_j ds[b][j] bank[idx[b][j]][d]."""
    rows = _f64(bank)[np.asarray(idx)]
    return np.einsum("br,brd->bd", _f64(ds), rows) * inv_T


def scores_grad_bound(bank, idx, ds, inv_T=INV_T):
    """bank_scores_bwd_kernel: a wave adds 16 rows per trip of 256 (a product and an add each: 32 roundings), ceil(R / 256)
    trips; then the sequential fold over the 16 waves (16 adds) and the product with 1/T: c = 32 ceil(R / 256) + 17.
    S = (1/T) sum_j |ds[b][j] row_j[d]|."""
    rows = _f64(bank)[np.asarray(idx)]
    S = np.einsum("br,brd->bd", np.abs(_f64(ds)), np.abs(rows)) * inv_T
    return (32 * math.ceil(rows.shape[1] / 256) + 17) * U * S


# ---- bank[y[i]] = normalize(m bank[y[i]] + (1 - m) emb[i]); the last duplicate wins -----------------------------------------
def bank_update(bank, y, emb, momentum):
    """(updated bank, per-element bound; 0 on the rows no sample owns: they must keep their bits).  The kernel takes the
    momentum as a float and forms 1 - m in float32, which is exact for m in [0.5, 1]: the reference uses those two values.

    bank_update_rows, t_d = fl(fl(p_d m) + fl(e_d (1 - m))) (explicitly unfused): |dt_d| <= 2 u T_d, T_d = |p_d m| + |e_d (1 - m)|.
    ss = sum t^2: (trips + 7) u relative from its own roundings (as in the normalize forward) + 2 sum |t| |dt| / ss
    = 4 kappa u from the inputs, kappa = sum |t_d| T_d / ss (>= 1; large when m p and (1 - m) e cancel).  The norm: half of that
    + the square root's rounding; the division adds one:
      |d out_d| <= u (2 T_d + c_n |t_d|) / norm,   c_n = (trips + 7) / 2 + 2 kappa + 2."""
    bank, emb, y = _f64(bank), _f64(emb), np.asarray(y)
    m = float(np.float32(momentum))
    out, bound = bank.copy(), np.zeros_like(bank)
    D = bank.shape[1]
    for i in range(len(y)):
        if (y[i + 1:] == y[i]).any():
            continue                                               # a later sample owns this row
        p, e = bank[y[i]], emb[i]
        t = p * m + e * (1.0 - m)
        T = np.abs(p * m) + np.abs(e * (1.0 - m))
        ss = (t * t).sum()
        n = max(math.sqrt(ss), 1e-12)
        kappa = (np.abs(t) * T).sum() / ss
        out[y[i]] = t / n
        bound[y[i]] = U * (2 * T + ((trips(D) + 7) / 2 + 2 * kappa + 2) * np.abs(t)) / n
    return out, bound


# ---- inputs (made once per shape, float32 CPU tensors; callers never modify them) -------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _signed(gen, shape, lo=0.5):
    """Magnitudes in [lo, 1) with random signs: every term carries real weight."""
    mag = lo + (1 - lo) * torch.rand(shape, generator=gen)
    return mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()


@functools.lru_cache(maxsize=None)
def l2_inputs(bs, D):
    """(x, dy).  The last element of every row has real weight in the norm, the last slice in <y, dy> (a dropped last slice
    shows even where it is one element wide); at bs = 5 row 3 is zero."""
    g = _gen(1, bs, D)
    x = torch.randn(bs, D, generator=g) * 3
    dy = torch.rand(bs, D, generator=g) * 2 - 1
    x[:, -1] = _signed(g, (bs,)) * 6
    cut = last_slice(D)
    dy[:, cut:] = (0.5 + dy[:, cut:].abs() / 2) * torch.sign(x[:, cut:])      # the last slice's terms of <y, dy> do not cancel
    if bs > L2_ZERO_ROW:
        x[L2_ZERO_ROW] = 0
    return x, dy


@functools.lru_cache(maxsize=None)
def score_inputs(D, bs, R, N=SCORE_N):
    """(bank [N, D], emb [bs, D], idx [bs, R] int64, ds [bs, R]).  Unit rows.  Sample b's LAST index points at bank row
    N - 1 - b, which is set equal to emb[b]: its score is 1/T, what a trained positive has, and the last row of every ragged
    block carries the largest weight.  Index 0 (and N - 1, through sample 0's positive) are present.  |ds| in [0.5, 1)."""
    g = _gen(2, D, bs, R)
    bank = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    emb = torch.nn.functional.normalize(torch.randn(bs, D, generator=g), dim=1)
    idx = torch.randint(1, N - bs, (bs, R), generator=g)
    for b in range(bs):
        bank[N - 1 - b] = emb[b]
        idx[b, R - 1] = N - 1 - b
        if R > 1:
            idx[b, 0] = 0
    ds = _signed(g, (bs, R))
    return bank, emb, idx, ds


@functools.lru_cache(maxsize=None)
def update_inputs(D, B, N=UPDATE_N):
    """(bank [N, D], emb0 [B, D], emb1 [B, D], y [B] int64).  Unit rows.  B >= 5: a triple duplicate id whose last
    occurrence is not the last sample, ids 0 and N - 1 present."""
    g = _gen(3, D, B)
    bank = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    emb0 = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    emb1 = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    y = 1 + torch.randperm(N - 2, generator=g)[:B]
    if B >= 5:
        first, second, third = (0, 2, 3) if B == 5 else (3, 7, 30)
        y[second] = y[first]
        y[third] = y[first]
        y[1] = 0
        y[B - 1] = N - 1
    return bank, emb0, emb1, y


def update_duplicates(B):
    return None if B < 5 else ((0, 2, 3) if B == 5 else (3, 7, 30))


# ---- the correspondence search --------------------------------------------------------------------------------------------
TOPK_WIDTHS = (64, 256)
TOPK_N = (500, 4608)                 # the exact scan; the threshold filter (banks of >= 4096 rows)
TOPK_K = 8
TOPK_KINDS = ("consensus", "union", "video", "audio")


@functools.lru_cache(maxsize=None)
def topk_banks(N, D):
    g = _gen(4, N, D)
    return (torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1),
            torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1))


def topk_tolerance(D):
    """What tests/test_gpu_knn.py allows a float32 (or split-bf16) dot product of two unit rows of width D: D 2^-22."""
    return D * 2.0 ** -22


def topk_check(N, D, got):
    """``got``: {kind: [N, K] rows found for every query}.  Against the float64 agreement scores of the banks of
    ``topk_banks(N, D)``, for every query and kind (tol = ``topk_tolerance(D)``, kth = its K-th best score after itself):
    K distinct rows in ascending order, never the query itself; every row scoring above kth + 2 tol is present; no row present
    scores below kth - 2 tol.  Returns {kind: (fraction of queries whose set is the float64 top-K, smallest number of rows a
    query has in common with it)}: what the rule of test_cma_topk_filter_path_vs_oracle bounds (> 0.998, >= K - 1)."""
    v1, v2 = (t.double() for t in topk_banks(N, D))
    K, tol = TOPK_K, topk_tolerance(D)
    stats = {}
    got = {k: torch.as_tensor(np.asarray(g)).long() for k, g in got.items()}
    for kind, g in got.items():
        assert tuple(g.shape) == (N, K) and int(g.min()) >= 0 and int(g.max()) < N, kind
        assert bool((g[:, 1:] > g[:, :-1]).all()), f"{kind}: rows not in ascending order"
        assert not bool((g == torch.arange(N)[:, None]).any()), f"{kind}: a query found itself"
    same = {k: 0 for k in got}
    common = {k: K for k in got}
    for q0 in range(0, N, 512):
        q1 = min(q0 + 512, N)
        vs, as_ = v1 @ v1[q0:q1].t(), v2 @ v2[q0:q1].t()
        for kind, g in got.items():
            sim = {"consensus": torch.minimum(vs, as_), "union": torch.maximum(vs, as_), "video": vs, "audio": as_}[kind]
            val, pidx = torch.topk(sim, K + 1, dim=0, sorted=True)
            assert bool((pidx[0] == torch.arange(q0, q1)).all())                 # rank 0 is the query itself
            kth = val[K]
            pair = sim.gather(0, g[q0:q1].t())
            assert bool((pair >= kth - 2 * tol).all()), f"{kind}: a row below the K-th best score by more than 2 tol"
            must = (sim > kth + 2 * tol).sum(0) - 1                              # (the query itself is one of them)
            assert bool(((pair > kth + 2 * tol).sum(0) == must).all()), f"{kind}: a row above the K-th best score is missing"
            want = pidx[1:].t().sort(dim=1).values
            eq = (g[q0:q1][:, :, None] == want[:, None, :]).any(2).sum(1)
            same[kind] += int((eq == K).sum())
            common[kind] = min(common[kind], int(eq.min()))
    for kind in got:
        stats[kind] = (same[kind] / N, common[kind])
    return stats


# ---- criterions.AVID / AVID_CMA at other widths: two steps with injected negatives ------------------------------------------
CRIT_WIDTHS = (64, 256)
CRIT = {"avid": dict(N=300, bs=4, K=16), "cma": dict(N=500, bs=4, K=64, Kw=16, pos_k=8)}
# The project's tolerances for these quantities (tests/test_gpu_model.py, test_avid_two_steps_vs_reference_golden): (rtol, atol)
CRIT_TOL = {"loss": (5e-6, 0.0), "Z": (5e-6, 0.0), "tb": (5e-6, 0.0), "grad": (2e-4, 2e-7), "rows": (2e-6, 2e-7)}


@functools.lru_cache(maxsize=None)
def crit_inputs(kind, D):
    """Banks, and per step the raw embeddings, the ids and the injected draw (AVID: the negatives; AVID_CMA: ``rand_idx``)."""
    c = CRIT[kind]
    g = _gen(5, len(kind), D)
    N, bs, K = c["N"], c["bs"], c["K"]
    v1 = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    v2 = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    steps = []
    for _ in range(2):
        v, a = torch.randn(bs, D, generator=g), torch.randn(bs, D, generator=g) * 0.5
        y = torch.randperm(N, generator=g)[:bs]
        if kind == "avid":
            draw = torch.randint(0, N - 1, (bs, K), generator=g)
            draw = draw + (draw >= y[:, None]).long()                       # never the sample itself
        else:
            draw = torch.randint(0, N - c["pos_k"], (bs, K), generator=g)
        steps.append((v, a, y, draw))
    return v1, v2, steps


def deviation(got, want, tol):
    """max |got - want| / (atol + rtol |want|): <= 1 passes ``assert_allclose(got, want, rtol, atol)``."""
    rtol, atol = tol
    got, want = _f64(got), _f64(want)
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


@functools.lru_cache(maxsize=None)
def oracle_steps(kind, D, dtype):
    """The two steps through the oracle (oracle/avid_oracle.py: the reference's formulas in torch on the CPU) in ``dtype``:
    per step {"loss", "Z", "tb": {...}, "gv", "ga", "v1rows", "v2rows"} as float64 numpy."""
    from oracle import avid_oracle as O
    v1, v2, steps = crit_inputs(kind, D)
    c = CRIT[kind]
    b1, b2 = v1.to(dtype).clone(), v2.to(dtype).clone()
    pset = torch.from_numpy(positive_set(D)) if kind == "cma" else None
    Z, out = None, []
    for v, a, y, draw in steps:
        vr, ar = v.to(dtype).clone().requires_grad_(True), a.to(dtype).clone().requires_grad_(True)
        if kind == "avid":
            loss, tb, Z = O.avid_forward(vr, ar, y, draw, b1, b2, Z=Z, momentum=0.5, xModal_coeff=1.0, wModal_coeff=1.0)
        else:
            loss, tb, Z = O.avid_cma_forward(vr, ar, y, draw, pset, b1, b2, Z=Z, momentum=0.5,
                                             num_negatives_within=c["Kw"], coeffs=(1.0, 1.0, 1.0, 1.0))
        loss.backward()
        out.append({"loss": float(loss.detach()), "Z": float(Z), "tb": {k: float(x.detach()) for k, x in tb.items()},
                    "gv": _f64(vr.grad), "ga": _f64(ar.grad), "v1rows": _f64(b1[y]), "v2rows": _f64(b2[y])})
    return out


@functools.lru_cache(maxsize=None)
def positive_set(D):
    """AVID_CMA's positive_set for the banks of ``crit_inputs("cma", D)``: the oracle's search (int32 [N, pos_k])."""
    from oracle import avid_oracle as O
    v1, v2, _ = crit_inputs("cma", D)
    return O.cma_topk(v1, v2, CRIT["cma"]["pos_k"], "consensus").astype(np.int32)
