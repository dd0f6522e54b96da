"""The graphs the Louvain tests share (tests/test_louvain_args.py, tests/test_gpu_louvain.py): small integer-weighted ones on which
every quantity of the rule is an integer below 2^53, and the float-weighted neighbour graphs of point clouds."""
import numpy as np
import scipy.sparse as sp

import neighbors_restatement as NR


def ring_of_cliques(cliques=8, size=5):
    """`cliques` complete graphs of `size` nodes, unit weights, the last node of each joined to the first of the next"""
    n = cliques * size
    A = np.zeros((n, n))
    for c in range(cliques):
        A[c * size:(c + 1) * size, c * size:(c + 1) * size] = 1.0
        a, b = c * size + size - 1, ((c + 1) * size) % n
        A[a, b] = A[b, a] = 1.0
    np.fill_diagonal(A, 0.0)
    return sp.csr_matrix(A)


def random_symmetric(n=193, mean_degree=6, seed=5):
    """symmetric, integer weights 1 .. 8"""
    rng = np.random.default_rng(seed)
    e = n * mean_degree // 2
    i, j = rng.integers(0, n, e), rng.integers(0, n, e)
    keep = i != j
    W = sp.coo_matrix((rng.integers(1, 9, e)[keep].astype(np.float64), (i[keep], j[keep])), shape=(n, n)).tocsr()
    W = W.maximum(W.T).tocsr()                     # (a pair drawn twice keeps one integer weight)
    return W


def directed_knn_ranks(n=300, k=5, seed=6):
    """A_ij = r when j is the r-th nearest neighbour of i among random 2-D points: unsymmetric"""
    X = np.random.default_rng(seed).uniform(size=(n, 2))
    idx = NR.knn(X, k)[0]
    return sp.csr_matrix((np.tile(np.arange(1.0, k + 1), n), idx.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))


def hub(n=200, hub_degree=150, seed=8):
    """a sparse symmetric rest (mean degree 4, weights 1 .. 4) and node 0 joined to `hub_degree` others with weight 1"""
    rng = np.random.default_rng(seed)
    W = random_symmetric(n, 4, seed).minimum(4.0).tolil()
    others = rng.choice(np.arange(1, n), hub_degree, replace=False)
    for j in others:
        W[0, j] = W[j, 0] = 1.0
    return W.tocsr()


# the degrees of nodes 0 .. 10 of tile_crossing(): one either side of every limit of the move kernels' degree bins and of the
# workgroup kernel's staging, sort and LDS sizes (DESIGN.md K17 lists which degree reaches which path)
LADDER = (63, 64, 65, 256, 257, 512, 513, 4096, 4097, 8192, 8193)


def tile_crossing(n=9000, seed=21):
    """random_symmetric(n, 6, seed) with nodes 0 .. 31 cut out of it; node t < 11 is then joined to LADDER[t] distinct nodes of
    32 .. n-1 with weights 1 .. 3, both directions; nodes 11 .. 31 stay isolated.  Symmetric, exact, largest other degree 19"""
    W = random_symmetric(n, 6, seed).tocoo()
    keep = (W.row >= 32) & (W.col >= 32)
    rows, cols, vals = [W.row[keep]], [W.col[keep]], [W.data[keep]]
    rng = np.random.default_rng(seed)
    for t, d in enumerate(LADDER):
        others = rng.choice(np.arange(32, n), d, replace=False)
        weights = rng.integers(1, 4, d).astype(np.float64)
        rows += [np.full(d, t), others]
        cols += [others, np.full(d, t)]
        vals += [weights, weights]
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


def odd_ends():
    """(raw CSR, n): isolated nodes (2, 9), a node whose only entry is a self-loop (5), a self-loop beside edges (0), repeated and
    unsorted columns (rows 0, 3, 7), a stored zero (row 4), two triangles and a tail; unsymmetric"""
    rows = {0: [(3, 2), (1, 1), (0, 4), (3, 1)], 1: [(0, 1), (3, 2)], 3: [(1, 2), (0, 1), (1, 1), (0, 2)], 4: [(6, 3), (7, 0), (8, 1)],
            5: [(5, 7)], 6: [(4, 3), (7, 2)], 7: [(6, 2), (4, 1), (6, 1), (8, 2)], 8: [(7, 1), (10, 1)], 10: [(8, 2), (11, 5)],
            11: [(10, 5)]}
    n = 12
    indptr, indices, data = [0], [], []
    for i in range(n):
        for j, v in rows.get(i, []):
            indices.append(j)
            data.append(float(v))
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(n, n)), n


def exact_enough(A):
    """every product of the rule stays an integer below 2^53: w^2 bounds them all"""
    A = sp.csr_matrix(A)
    w = float(A.data.sum())
    return np.array_equal(A.data, np.round(A.data)) and w * w < 2.0 ** 53


# the planted partition: 6 Gaussian blobs in 10-D, unit spread, centres drawn N(0, BLOB_SEPARATION^2) per coordinate.  At 3.0 (and at
# 4.0 and 6.0) the synchronous restatement and the sequential reference return the same partition, the planted one, on the
# 15-neighbour graph in both modes (measured on the CPU: Q = 0.83332 in both).
BLOB_SEPARATION = 3.0


def blobs(n=1500, k=6, D=10, seed=7):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(k, D)) * BLOB_SEPARATION
    planted = np.arange(n) % k
    return centres[planted] + rng.normal(size=(n, D)), planted


def uniform_union_graph(n=1000, n_neighbors=15, seed=11):
    """the fuzzy union of the 14 nearest neighbours of uniform 2-D points (what tl.neighbors calls connectivities): no structure"""
    X = np.random.default_rng(seed).uniform(size=(n, 2))
    idx, dist, _ = NR.knn(X, n_neighbors - 1)
    return NR.connectivities(idx, dist, n_neighbors)


def same_partition(a, b):
    a, b = np.asarray(a).tolist(), np.asarray(b).tolist()
    return len(set(zip(a, b))) == len(set(a)) == len(set(b))


def numbered_by_size(labels):
    """labels are 0 .. k-1, by decreasing size, ties to the smallest member"""
    labels = np.asarray(labels)
    ids, first, counts = np.unique(labels, return_index=True, return_counts=True)
    if not np.array_equal(ids, np.arange(ids.size)):
        return False
    return all((counts[c] > counts[c + 1]) or (counts[c] == counts[c + 1] and first[c] < first[c + 1]) for c in range(ids.size - 1))
