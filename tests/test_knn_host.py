"""k-NN evaluation without a GPU: the float64 restatement the kernels are held to (tests/_knn_ref.py) against torch.topk and
its tie rule, the C ABI's declarations and argument validation, and ``KNNEval``'s host logic over the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _knn_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -4


def test_restatement_equals_float64_topk_without_ties():
    rng = np.random.default_rng(0)
    g, q = rng.standard_normal((300, 32)), rng.standard_normal((17, 32))
    idx, sim = R.search(g, q, 20)
    s = torch.from_numpy(q) @ torch.from_numpy(g).T
    assert all(len(np.unique(row)) == len(row) for row in s.numpy()), "the inputs were meant to be tie-free"
    tv, ti = torch.topk(s, 20, dim=1)
    assert np.array_equal(idx, ti.numpy().astype(np.int32))
    # (two float64 matrix products: they differ by the summation order, 32 terms of magnitude <= |q| |g|)
    assert np.abs(sim - tv.numpy()).max() <= 32 * 2.0 ** -52 * float(s.abs().max())
    # exclude: the named row leaves, the rest keep their order; -1 and a row outside the best k + 1 drop the last one
    ex = np.where(np.arange(17) % 3 == 0, idx[:, 2], -1).astype(np.int32)
    ex[1] = int(torch.argmin(s[1]))
    idx2, sim2 = R.search(g, q, 19, exclude=ex)
    for r in range(17):
        keep = [j for j in range(20) if idx[r, j] != ex[r]][:19]
        assert np.array_equal(idx2[r], idx[r, keep]) and np.array_equal(sim2[r], sim[r, keep])


def test_restatement_orders_ties_by_index():
    rng = np.random.default_rng(1)
    base = rng.standard_normal((40, 32))
    g = np.concatenate([base, base[:25], base[:25]], 0)           # rows n, 40 + n, 65 + n are identical (n < 25)
    q = base[:6] * 3.0
    idx, sim = R.search(g, q, 7)
    for r in range(6):
        assert np.all(np.diff(sim[r]) <= 0)
        for a, b in zip(range(6), range(1, 7)):
            if sim[r, a] == sim[r, b]:
                assert idx[r, a] < idx[r, b]
        assert list(idx[r, :3]) == [r, 40 + r, 65 + r]             # the query's own direction: three equal best rows
    # a tie across the k-th rank: the smaller index stays
    idx2, _ = R.search(g, q, 2)
    assert [list(x) for x in idx2] == [[r, 40 + r] for r in range(6)]
    idx3, _ = R.search(g, q, 2, exclude=np.array([40 + r for r in range(6)], np.int32))
    assert [list(x) for x in idx3] == [[r, 65 + r] for r in range(6)]


def test_vote_restatement():
    idx = np.array([[3, 0, 2], [1, 1, 1]], np.int32)
    sim = np.array([[0.9, 0.5, 0.5], [0.1, 0.1, 0.1]])
    labels = np.array([1, 0, 1, 2], np.int32)
    scores, p5, first = R.vote(idx, sim, labels, 3, T=0.5, query_labels=np.array([1, 2], np.int32))
    e = np.exp
    assert np.allclose(scores, [[0, e(1.0) + e(1.0), e(1.8)], [3 * e(0.2), 0, 0]])
    assert p5.tolist() == [[2, 1, 0, -1, -1], [0, 1, 2, -1, -1]] and first.tolist() == [1, 3]
    assert R.pred5(np.array([[1.0, 3.0, 3.0, 0.0, 2.0, 3.0, 0.0]])).tolist() == [[1, 2, 5, 4, 0]]


def test_symbols_are_declared_and_bound():
    from avid_hip import lib
    header = open(os.path.join(REPO, "include", "avid_hip.h")).read()
    for name in ("avid_knn_workspace_bytes", "avid_knn_search", "avid_knn_vote"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SIGNATURES and hasattr(lib.raw(name), "argtypes")
    assert len(lib.SIGNATURES["avid_knn_search"][1]) == 13 and len(lib.SIGNATURES["avid_knn_vote"][1]) == 13
    assert lib.version() >= 161


def test_search_validates_its_arguments_before_any_launch():
    from avid_hip import lib
    run, need = lib.raw("avid_knn_search"), lib.raw("avid_knn_workspace_bytes")
    buf = (C.c_float * 64)()                                      # never dereferenced: every call below is refused
    p = C.cast(buf, C.c_void_p)

    def call(N=4096, D=128, gallery=p, queries=p, nq=128, k=20, exclude=None, out_idx=p, out_sim=p, ws=p, ws_bytes=None):
        nb = need(N, nq, k) if ws_bytes is None else ws_bytes
        return run(N, D, gallery, queries, nq, k, exclude, out_idx, out_sim, None, ws, nb or (1 << 40), None)

    for arg in ("gallery", "queries", "out_idx", "out_sim", "ws"):
        assert call(**{arg: None}) == BADARG and "null pointer" in lib.last_error(), arg
    assert call(k=64, exclude=p) == UNSUPPORTED and "exclude" in lib.last_error()
    assert call(k=65) == UNSUPPORTED and call(k=0) == UNSUPPORTED
    assert call(nq=70) == UNSUPPORTED and "nq" in lib.last_error()
    assert call(D=48) == UNSUPPORTED
    assert call(N=63) == UNSUPPORTED and "64 <= N" in lib.last_error()
    assert call(N=1 << 31) == UNSUPPORTED
    assert call(ws_bytes=need(4096, 128, 20) - 1) == BADARG and "workspace too small" in lib.last_error()
    # the workspace query: 0 for what the search refuses, the score slab and more otherwise
    assert need(63, 128, 20) == 0 and need(4096, 70, 20) == 0 and need(4096, 128, 65) == 0 and need(4096, 128, 0) == 0
    assert need(4096, 128, 20) > 4 * 4096 * 128 and need(4096, 128, 64) > 0
    assert need(200, 64, 63) > 4 * 200 * 64


def test_vote_validates_its_arguments_before_any_launch():
    from avid_hip import lib
    run = lib.raw("avid_knn_vote")
    p = C.cast((C.c_float * 64)(), C.c_void_p)

    def call(nq=64, k=20, idx=p, sim=p, labels=p, N=4096, n_classes=101, inv_T=1 / 0.07, ql=None, scores=p, pred5=p, first=None):
        return run(nq, k, idx, sim, labels, N, n_classes, inv_T, ql, scores, pred5, first, None)

    for arg in ("idx", "sim", "labels", "scores", "pred5"):
        assert call(**{arg: None}) == BADARG and "null pointer" in lib.last_error(), arg
    assert call(ql=p, first=None) == BADARG and "first_match" in lib.last_error()
    assert call(nq=0) == BADARG and call(N=0) == BADARG
    assert call(k=0) == UNSUPPORTED and call(k=65) == UNSUPPORTED
    assert call(n_classes=0) == UNSUPPORTED and call(n_classes=8193) == UNSUPPORTED


def test_ops_refuse_cpu_and_mistyped_tensors():
    from avid_hip import ops
    from avid_hip.lib import AvidHipError
    g, q = torch.zeros(64, 32), torch.zeros(3, 32)
    with pytest.raises(AvidHipError, match="device tensor"):
        ops.knn_search(g, q, 5)
    with pytest.raises(AvidHipError, match="device tensor"):
        ops.knn_vote(torch.zeros(3, 5, dtype=torch.int32), torch.zeros(3, 5), torch.zeros(64, dtype=torch.int32), 4)


# ---- KNNEval's host logic over the restatement ------------------------------------------------------------------------
@pytest.fixture
def ref_ops(monkeypatch):
    """``ops.knn_search`` / ``ops.knn_vote`` replaced by the restatement on CPU tensors; the calls are recorded."""
    from avid_hip import ops
    calls = []

    def search(gallery, queries, k, exclude=None, batch=128, fallbacks=None):
        calls.append(("search", gallery.clone(), queries.clone(), k, None if exclude is None else exclude.clone()))
        idx, sim = R.search(gallery.numpy(), queries.numpy(), k, None if exclude is None else exclude.numpy())
        return torch.from_numpy(idx), torch.from_numpy(sim.astype(np.float32))

    def vote(idx, sim, gallery_labels, n_classes, T=0.07, query_labels=None):
        calls.append(("vote", n_classes, T, gallery_labels.clone(), None if query_labels is None else query_labels.clone()))
        assert gallery_labels.dtype == torch.int32 and (query_labels is None or query_labels.dtype == torch.int32)
        s, p5, first = R.vote(idx.numpy(), sim.numpy(), gallery_labels.numpy(), n_classes, T,
                              None if query_labels is None else query_labels.numpy())
        return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(p5), None if first is None else torch.from_numpy(first)

    monkeypatch.setattr(ops, "knn_search", search)
    monkeypatch.setattr(ops, "knn_vote", vote)
    return calls


def _planted(seed, n_classes, per_class, D=32, noise=0.05):
    """Class prototypes (the same for every seed) plus small noise (the seed's)."""
    protos = torch.nn.functional.normalize(torch.randn(n_classes, D, generator=torch.Generator().manual_seed(99)), dim=1)
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(n_classes).repeat_interleave(per_class)
    return protos[labels] + noise * torch.randn(len(labels), D, generator=g), labels


def test_knneval_counts_over_the_restatement(ref_ops):
    from avid_hip import parallel
    feats, labels = _planted(0, 6, 12)
    ev = parallel.KNNEval(k=10, T=0.07, n_classes=6, normalize=False)
    ev.add_gallery_features(feats[:40], labels[:40])
    ev.add_gallery_features(feats[40:], labels[40:].to(torch.int32))
    gal, gl = ev.gallery()
    assert torch.equal(gal, feats) and gl.dtype == torch.int32 and torch.equal(gl.long(), labels)
    assert ev.gallery()[0] is gal                                  # concatenated once
    q, ql = _planted(1, 6, 3)
    ql[0], ql[5] = 3, 0                                            # two queries mislabelled: they must miss
    out = ev.evaluate(q, ql, recall_at=(1, 5, 10, 20, 50))
    idx, sim = R.search(feats.numpy(), q.numpy(), 10)
    scores, p5, first = R.vote(idx, sim.astype(np.float32), labels.numpy(), 6, 0.07, ql.numpy())
    assert int(out["n"]) == 18 and out["n"].dtype == torch.int64
    assert int(out["top1_hits"]) == int((p5[:, 0] == ql.numpy()).sum()) == 16
    assert int(out["top5_hits"]) == int((p5 == ql.numpy()[:, None]).any(1).sum())
    assert sorted(out["recall_hits"]) == [1, 5, 10]                # entries above k are dropped
    for r in (1, 5, 10):
        assert int(out["recall_hits"][r]) == int((first < r).sum())
    assert int(out["recall_hits"][1]) == 16
    kind, g_, q_, k_, ex_ = ref_ops[0]
    assert kind == "search" and k_ == 10 and ex_ is None and torch.equal(q_, q)
    assert ref_ops[1][1:3] == (6, 0.07)


def test_knneval_averages_clips_in_the_tiling_order(ref_ops):
    from avid_hip import parallel
    feats, labels = _planted(2, 4, 16)
    ev = parallel.KNNEval(k=5, n_classes=4, normalize=False)
    ev.add_gallery_features(feats, labels)
    g = torch.Generator().manual_seed(3)
    clips = torch.randn(7 * 3, 32, generator=g)                    # 7 samples x 3 clips, a sample's clips adjacent
    ql = torch.randint(0, 4, (7,), generator=g)
    ev.evaluate(clips, ql, clips_per_sample=3)
    q_seen = ref_ops[0][2]
    assert q_seen.shape == (7, 32) and torch.equal(q_seen, clips.view(7, 3, 32).mean(1))
    assert not torch.equal(q_seen, clips.view(3, 7, 32).mean(0))
    with pytest.raises(ValueError, match="multiple of clips_per_sample"):
        ev.evaluate(clips[:20], ql, clips_per_sample=3)
    with pytest.raises(ValueError, match="labels"):
        ev.evaluate(clips, ql, clips_per_sample=1)
    with pytest.raises(ValueError, match="labels"):
        ev.evaluate(clips, ql.float()[:7], clips_per_sample=3)


def test_knneval_leave_one_out(ref_ops):
    from avid_hip import parallel
    feats, labels = _planted(4, 5, 14)
    ev = parallel.KNNEval(k=8, n_classes=5, normalize=False)
    ev.add_gallery_features(feats, labels)
    out = ev.evaluate(leave_one_out=True, recall_at=(1, 8, 9))
    kind, g_, q_, k_, ex_ = ref_ops[0]
    assert torch.equal(g_, q_) and ex_.dtype == torch.int32 and torch.equal(ex_, torch.arange(70, dtype=torch.int32))
    assert torch.equal(ref_ops[1][3], ref_ops[1][4])              # the gallery's labels are the queries'
    assert int(out["n"]) == 70 and int(out["top1_hits"]) == 70 and sorted(out["recall_hits"]) == [1, 8]
    with pytest.raises(ValueError, match="leave_one_out"):
        ev.evaluate(feats, labels, leave_one_out=True)


def test_knneval_refuses_what_it_cannot_do():
    from avid_hip import parallel
    with pytest.raises(ValueError):
        parallel.KNNEval(k=20)                                     # n_classes is required
    with pytest.raises(ValueError):
        parallel.KNNEval(k=64, n_classes=10)
    with pytest.raises(ValueError):
        parallel.KNNEval(feat="conv5x", n_classes=10)
    ev = parallel.KNNEval(n_classes=10, normalize=False)
    with pytest.raises(ValueError, match="empty"):
        ev.evaluate(torch.zeros(2, 32), torch.zeros(2, dtype=torch.int64))
    ev.add_gallery_features(torch.zeros(64, 32), torch.zeros(64, dtype=torch.int64))
    with pytest.raises(ValueError, match="without a model"):
        ev.evaluate(torch.zeros(2, 3, 8, 48, 48), torch.zeros(2, dtype=torch.int64))
