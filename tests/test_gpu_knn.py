"""k-NN search and vote on the GPU (``avid_knn_search`` / ``avid_knn_vote`` through ``ops.knn_search`` / ``ops.knn_vote``) against
the float64 restatement of tests/_knn_ref.py, and ``KNNEval`` end to end.  The shapes are the smallest that reach each path: 200
gallery rows for the exact scan, 4133 (no multiple of anything) for the threshold filter, 70 and 130 queries for a shifted last
batch, 5 for a padded one."""
import functools

import numpy as np
import pytest
import torch

import _knn_ref as R
from _inference_probe import wrapper

pytestmark = pytest.mark.gpu


# ---- exact arithmetic: every product and sum is exact in fp32 (and in the split-bf16 products), ties abound ------------------
@functools.lru_cache(maxsize=None)
def _lattice(N, Q):
    """Features from {-4..4} / 8, D = 32; an exclude vector with every kind of entry."""
    rng = np.random.default_rng(N + Q)
    g = rng.integers(-4, 5, (N, 32)).astype(np.float32) / 8
    q = rng.integers(-4, 5, (Q, 32)).astype(np.float32) / 8
    best = R.search(g, q, 8)[0]
    ex = np.full(Q, -1, np.int32)                                  # q % 4 == 1: none
    ex[0::4] = best[0::4, 0]                                       # the best row
    ex[2::4] = best[2::4, 5]                                       # a row inside the best k + 1 (for k >= 5)
    ex[3::4] = rng.integers(0, N, len(ex[3::4]))                   # some row, mostly far down
    return g, q, ex


@functools.lru_cache(maxsize=None)
def _lattice_ref(N, Q, k, excl):
    g, q, ex = _lattice(N, Q)
    return R.search(g, q, k, ex if excl else None)


@pytest.mark.parametrize("excl", [False, True], ids=["all", "exclude"])
@pytest.mark.parametrize("k", [1, 20, 63])
@pytest.mark.parametrize("N,Q", [(200, 70), (4133, 130)])
def test_search_is_exact_on_lattice_features(N, Q, k, excl, gpu_device):
    from avid_hip import ops
    g, q, ex = _lattice(N, Q)
    want_i, want_s = _lattice_ref(N, Q, k, excl)
    # the inputs exercise the tie rule: for some query the k-th and the (k + 1)-th best score are equal
    wide = _lattice_ref(N, Q, k + 1, False)[1]
    assert (wide[:, k - 1] == wide[:, k]).any(), "no tie at the k-th rank in these inputs"
    fb = torch.zeros((), dtype=torch.int32, device=gpu_device)
    idx, sim = ops.knn_search(torch.from_numpy(g).to(gpu_device), torch.from_numpy(q).to(gpu_device), k,
                              exclude=torch.from_numpy(ex).to(gpu_device) if excl else None, fallbacks=fb)
    assert idx.shape == (Q, k) and idx.dtype == torch.int32 and sim.dtype == torch.float32
    print(f"N {N} Q {Q} k {k} exclude {excl}: fallbacks {int(fb)}")
    assert torch.equal(idx.cpu(), torch.from_numpy(want_i))
    assert torch.equal(sim.cpu(), torch.from_numpy(want_s.astype(np.float32)))
    if excl:
        assert not (idx.cpu() == torch.from_numpy(ex)[:, None]).any()
    assert int(fb) == 0                                            # (at most 520 candidates per query, counted on the CPU)


def test_rows_do_not_depend_on_their_batch(gpu_device):
    """130 queries in batches of 128 (one shifted back) and of 64 (two and a shifted one), 5 queries padded to 64: the same rows."""
    from avid_hip import ops
    g, q, ex = (torch.from_numpy(a).to(gpu_device) for a in _lattice(4133, 130))
    a = ops.knn_search(g, q, 20, exclude=ex, batch=128)
    b = ops.knn_search(g, q, 20, exclude=ex, batch=64)
    c = ops.knn_search(g, q[:5].contiguous(), 20, exclude=ex[:5].contiguous())
    d = ops.knn_search(g, q[129:].contiguous(), 20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(c[0], a[0][:5]) and torch.equal(c[1], a[1][:5]) and c[0].shape == (5, 20)
    want = _lattice_ref(4133, 130, 20, False)
    assert torch.equal(d[0].cpu(), torch.from_numpy(want[0][129:])) and d[0].shape == (1, 20)


@pytest.mark.parametrize("excl", [False, True], ids=["all", "exclude"])
def test_overflowing_candidate_lists_fall_back_to_the_exact_scan(excl, gpu_device):
    """1500 identical gallery rows that are every query's best match (all entries 1/2 against positive queries): they all reach
    the threshold, 1500 > the 1024 candidate slots, the batch is redone by the exact scan — and the answer is the 20 of them
    with the smallest indices."""
    from avid_hip import ops
    rng = np.random.default_rng(7)
    N, Q, k = 4160, 130, 20
    g = rng.integers(-4, 5, (N, 32)).astype(np.float32) / 8
    dup = np.sort(rng.permutation(N)[:1500])
    g[dup] = 0.5
    q = rng.integers(1, 5, (Q, 32)).astype(np.float32) / 8
    ex = np.where(np.arange(Q) % 2 == 0, dup[np.arange(Q) % 7], -1).astype(np.int32) if excl else None
    want_i, want_s = R.search(g, q, k, ex)
    assert np.isin(want_i, dup).all()
    fb = torch.zeros((), dtype=torch.int32, device=gpu_device)
    idx, sim = ops.knn_search(torch.from_numpy(g).to(gpu_device), torch.from_numpy(q).to(gpu_device), k,
                              exclude=None if ex is None else torch.from_numpy(ex).to(gpu_device), fallbacks=fb)
    print("fallbacks", int(fb))
    assert int(fb) == 2                                            # both batches of 128
    assert torch.equal(idx.cpu(), torch.from_numpy(want_i)) and torch.equal(sim.cpu(), torch.from_numpy(want_s.astype(np.float32)))


# ---- random unit vectors: fp32 rounding decides near-ties, so the question is containment within a tolerance ---------------
@functools.lru_cache(maxsize=None)
def _unit(D):
    gen = torch.Generator().manual_seed(D)
    g = torch.nn.functional.normalize(torch.randn(4133, D, generator=gen), dim=1)
    q = torch.nn.functional.normalize(torch.randn(130, D, generator=gen), dim=1)
    return g, q, q.double().numpy() @ g.double().numpy().T


@functools.lru_cache(maxsize=None)
def _unit_result(D, k):
    from avid_hip import ops
    g, q, _ = _unit(D)
    idx, sim = ops.knn_search(g.cuda(), q.cuda(), k)
    return idx, sim


@pytest.mark.parametrize("D", [128, 512])
def test_search_on_random_unit_vectors(D, gpu_device):
    k, tol = 20, D * 2.0 ** -22
    _, _, s64 = _unit(D)
    idx, sim = (t.cpu().numpy() for t in _unit_result(D, k))
    assert idx.min() >= 0 and idx.max() < 4133 and all(len(set(r)) == k for r in idx)
    assert (np.diff(sim, axis=1) <= 0).all()
    pair = np.take_along_axis(s64, idx.astype(np.int64), 1)
    err = np.abs(sim - pair).max()
    print(f"D {D}: largest |sim - float64 dot| {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    kth = -np.sort(-s64, axis=1)[:, k - 1]
    must = s64 > (kth + 2 * tol)[:, None]
    present = np.zeros_like(must)
    np.put_along_axis(present, idx.astype(np.int64), True, 1)
    assert not (must & ~present).any()
    assert (pair >= (kth - 2 * tol)[:, None]).all()


# ---- the vote --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes,k", [(3, 20), (101, 20), (3, 63)])
def test_vote_matches_the_restatement(n_classes, k, gpu_device):
    from avid_hip import ops
    idx, sim = _unit_result(128, k)
    rng = np.random.default_rng(n_classes)
    gl = rng.integers(0, n_classes, 4133).astype(np.int32)
    ql = rng.integers(0, n_classes, 130).astype(np.int32)
    scores, pred5, first = ops.knn_vote(idx, sim, torch.from_numpy(gl).to(gpu_device), n_classes, T=0.07,
                                        query_labels=torch.from_numpy(ql).to(gpu_device))
    want, _, want_first = R.vote(idx.cpu().numpy(), sim.cpu().numpy(), gl, n_classes, 0.07, ql)
    got = scores.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (130, n_classes)
    rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print(f"classes {n_classes} k {k}: largest relative error of a score {rel.max():.3e}")
    assert rel.max() <= 1e-5 and ((want == 0) == (got == 0)).all()
    assert np.array_equal(pred5.cpu().numpy(), R.pred5(got))       # a stable descending sort of the device's own scores
    assert np.array_equal(first.cpu().numpy(), want_first)
    s2, p2, none = ops.knn_vote(idx, sim, torch.from_numpy(gl).to(gpu_device), n_classes, T=0.07)
    assert none is None and torch.equal(s2, scores) and torch.equal(p2, pred5)


# ---- KNNEval ---------------------------------------------------------------------------------------------------------------
def _counts(out):
    return (int(out["n"]), int(out["top1_hits"]), int(out["top5_hits"]), {r: int(v) for r, v in out["recall_hits"].items()})


def test_knneval_equals_the_ops_on_inference_features(gpu_device):
    """R2Plus1D-18 on 3x8x48x48 clips, two clips per sample: 8 gallery batches of 8 samples, one query batch of 5."""
    from avid_hip import ops, parallel
    m = wrapper(gpu_device, seed=21).feature_extractor
    gen = torch.Generator().manual_seed(22)
    gal = [torch.randn((8, 2, 3, 8, 48, 48), generator=gen).to(gpu_device) for _ in range(8)]
    gal_l = [torch.randint(0, 7, (8,), generator=gen).to(gpu_device) for _ in range(8)]
    qv, ql = torch.randn((5, 2, 3, 8, 48, 48), generator=gen).to(gpu_device), torch.randint(0, 7, (5,), generator=gen).to(gpu_device)
    ev = parallel.KNNEval(m, k=20, T=0.07, n_classes=7)
    for v, l in zip(gal, gal_l):
        ev.add_gallery(v, l, clips_per_sample=2)
    out = ev.evaluate(qv.flatten(0, 1), ql, clips_per_sample=2)    # (the flat tiling order; the gallery came as [B, clips, ...])
    assert all(t.is_cuda and t.dtype == torch.int64 for t in (out["n"], out["top1_hits"], out["top5_hits"], *out["recall_hits"].values()))
    assert sorted(out["recall_hits"]) == [1, 5, 10, 20]

    infer = parallel.Inference(m)

    def feats(v):
        f = infer(v.flatten(0, 1).contiguous()).flatten(1)
        assert f.shape[1] == 512
        return ops.l2_normalize(f.view(-1, 2, 512).mean(1).contiguous())
    G, GL = torch.cat([feats(v) for v in gal], 0), torch.cat(gal_l).to(torch.int32)
    assert torch.equal(ev.gallery()[0], G) and torch.equal(ev.gallery()[1], GL)
    idx, sim = ops.knn_search(G, feats(qv), 20)
    _, p5, first = ops.knn_vote(idx, sim, GL, 7, T=0.07, query_labels=ql.to(torch.int32))
    want = (5, int((p5[:, 0] == ql).sum()), int((p5 == ql[:, None]).any(1).sum()), {r: int((first < r).sum()) for r in (1, 5, 10, 20)})
    assert _counts(out) == want
    assert all(mod.training for mod in m.modules())


def test_knneval_on_planted_features(gpu_device, monkeypatch):
    """Class prototypes plus small noise, separable (checked here in float64): every query finds its class, and leave-one-out
    never returns the query's own row."""
    from avid_hip import ops, parallel
    gen = torch.Generator().manual_seed(5)
    protos = torch.nn.functional.normalize(torch.randn(10, 64, generator=gen), dim=1)
    gl, ql = torch.arange(10).repeat_interleave(20), torch.arange(10).repeat_interleave(7)
    G, Qf = protos[gl] + 0.02 * torch.randn(200, 64, generator=gen), protos[ql] + 0.02 * torch.randn(70, 64, generator=gen)
    for X, xl in ((Qf, ql), (G, gl)):                              # separable: every other-class row is well below every own-class row
        s = torch.nn.functional.normalize(X.double(), dim=1) @ torch.nn.functional.normalize(G.double(), dim=1).T
        own = xl[:, None] == gl[None, :]
        assert float(s.masked_fill(~own, 9).min(1).values.min()) - float(s.masked_fill(own, -9).max(1).values.max()) > 0.1
    ev = parallel.KNNEval(k=10, n_classes=10)
    ev.add_gallery_features(G[:90].to(gpu_device), gl[:90].to(gpu_device))
    ev.add_gallery_features(G[90:].to(gpu_device), gl[90:].to(gpu_device))
    n, top1, top5, recall = _counts(ev.evaluate(Qf.to(gpu_device), ql.to(gpu_device)))
    assert (n, top1, top5) == (70, 70, 70) and recall == {1: 70, 5: 70, 10: 70}
    seen = []
    search = ops.knn_search
    monkeypatch.setattr(ops, "knn_search", lambda *a, **kw: seen.append(search(*a, **kw)) or seen[-1])
    n, top1, top5, recall = _counts(ev.evaluate(leave_one_out=True, recall_at=(1, 20)))
    assert (n, top1, top5) == (200, 200, 200) and recall == {1: 200}
    idx, sim = seen[0]
    assert idx.shape == (200, 10) and not (idx == torch.arange(200, device=gpu_device)[:, None]).any()
    # without the exclusion the query's own row is its best match
    idx0, _ = search(ev.gallery()[0], ev.gallery()[0], 10)
    assert torch.equal(idx0[:, 0].cpu(), torch.arange(200, dtype=torch.int32))
    assert torch.equal(idx0[:, 1:], idx[:, :9])
