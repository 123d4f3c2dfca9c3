"""float64 restatement of the k-NN search and vote (``avid_knn_search`` / ``avid_knn_vote``), in numpy: what the HIP kernels
are held to.  Nothing here is shared with the code under test."""
import numpy as np


def search(gallery, queries, k, exclude=None):
    """(idx int32 [Q, k], sim float64 [Q, k]): per query the k gallery rows of largest float64 dot product, ordered by
    (similarity descending, gallery index ascending).  ``exclude[q]`` (-1: none): k + 1 rows are selected, that row removed
    where it is among them, the last one otherwise."""
    g, qs = np.asarray(gallery, np.float64), np.asarray(queries, np.float64)
    s = qs @ g.T
    K = k + (1 if exclude is not None else 0)
    idx = np.empty((len(qs), k), np.int32)
    sim = np.empty((len(qs), k), np.float64)
    rows = np.arange(len(g))
    for q in range(len(qs)):
        order = np.lexsort((rows, -s[q]))[:K]              # primary key: -score; ties: the smaller index first
        if exclude is not None:
            hit = np.nonzero(order == int(exclude[q]))[0]
            order = np.delete(order, hit[0] if len(hit) else K - 1)
        idx[q], sim[q] = order, s[q, order]
    return idx, sim


def vote(idx, sim, gallery_labels, n_classes, T=0.07, query_labels=None):
    """(scores float64 [Q, C], pred5 int32 [Q, 5], first_match int32 [Q] or None)."""
    idx, sim, gl = np.asarray(idx), np.asarray(sim, np.float64), np.asarray(gallery_labels)
    Q, k = idx.shape
    scores = np.zeros((Q, n_classes), np.float64)
    first = np.full(Q, k, np.int32) if query_labels is not None else None
    for q in range(Q):
        for j in range(k):                                 # rank order
            c = int(gl[idx[q, j]])
            scores[q, c] += np.exp(sim[q, j] / T)
            if first is not None and first[q] == k and c == int(query_labels[q]):
                first[q] = j
    return scores, pred5(scores), first


def pred5(scores):
    """The five best classes by (score descending, class ascending), padded with -1 below five classes."""
    scores = np.asarray(scores)
    Q, C = scores.shape
    out = np.full((Q, 5), -1, np.int32)
    order = np.argsort(-scores, axis=1, kind="stable")[:, :5]
    out[:, :order.shape[1]] = order
    return out
