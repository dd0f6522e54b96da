"""Synchronous Louvain (K17) restated in numpy, the plain way: Python loops over nodes, dictionaries for the coarse graph.  This file
is the rule the device is held to (pilot_amd/csrc/louvain_kernels.hpp states the same one); it is independent of the device code.
Also here: a modularity that uses neither S nor the scaled form, and a classic sequential Louvain as the quality reference.

The rule.  A: n x n, weights finite and >= 0, maybe unsymmetric; stored zeros dropped, repeats added.  out_i = sum_j A_ij,
in_i = sum_j A_ji, w = sum_i out_i, S = A + A^T (S_ii = 2 A_ii).  Qs = (w / 2) sum_{c_i = c_j} S_ij - gamma sum_c Out_c In_c and
Q = Qs / w^2 (Dugue-Perez; Newman's for a symmetric A).  A level starts from singletons; a sweep moves every node against ONE
snapshot: node i in X looks at every community C != X holding a stored neighbour j != i, k_C = sum_{j in C, j != i} S_ij (k_X alike,
0 without one),

    g(C) = w (k_C - k_X) - gamma (out_i (In_C - (In_X - in_i)) + in_i (Out_C - (Out_X - out_i)))

every product and sum rounded on its own; the candidate is the largest g, ties to the lowest C; i moves iff g > 0, except that a
singleton never moves to a singleton of higher id.  No move: the level ends.  Else the sweep is kept iff Qs_new - Qs_kept > tol w^2,
otherwise discarded and the level ends; at most 128 sweeps.  Aggregation: surviving ids ranked ascending, S' = P^T S P (internal
weight on the diagonal, never read as a neighbour), out' / in' the member sums; stop when a level merges nothing or after
max_levels.  Labels: 0 .. k-1 by decreasing size, ties to the smallest member.

Sum orders (as DESIGN.md K17 states them): k_C over a row's stored columns ascending; Out_c / In_c over members ascending; the two
sums of Qs over nodes / community ids with :func:`ordered_sum`; a coarse weight over the fine edges in (row, column) order."""
import numpy as np
import scipy.sparse as sp

MAX_SWEEPS, CHUNK = 128, 256


def ordered_sum(x):
    """x[0] + x[1] + ... inside every chunk of 256 consecutive entries, then the chunk sums in ascending order"""
    total = 0.0
    for c0 in range(0, len(x), CHUNK):
        part = 0.0
        for v in x[c0:c0 + CHUNK]:
            part = part + float(v)
        total = total + part
    return total


def as_csr(graph):
    """A as a canonical float64 CSR: repeats added, columns sorted, stored zeros dropped"""
    A = sp.csr_matrix(graph, dtype=np.float64, copy=True)
    if A.shape[0] != A.shape[1]:
        raise ValueError("square")
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    if A.nnz and (not np.isfinite(A.data).all() or A.data.min() < 0):
        raise ValueError("weights")
    return A


def degrees(A):
    out = np.asarray(A.sum(axis=1)).ravel()
    inn = np.asarray(A.sum(axis=0)).ravel()
    return out, inn, float(out.sum())


def modularity(graph, labels, gamma=1.0):
    """independent of the run: sum_same A_ij / w - gamma sum_c Out_c In_c / w^2, straight from A"""
    A = as_csr(graph).tocoo()
    labels = np.asarray(labels)
    w = A.data.sum()
    if w == 0:
        return 0.0
    k = int(labels.max()) + 1
    Out = np.bincount(labels[A.row], weights=A.data, minlength=k)
    In = np.bincount(labels[A.col], weights=A.data, minlength=k)
    same = A.data[labels[A.row] == labels[A.col]].sum()
    return float(same / w - gamma * (Out * In).sum() / (w * w))


class _Level:
    """the symmetric graph of one level as CSR rows (columns ascending), with its out / in weights"""

    def __init__(self, indptr, indices, data, out, inn):
        self.indptr, self.indices, self.data, self.out, self.inn = indptr, indices, data, out, inn
        self.m = len(out)

    def row(self, i):
        s = slice(self.indptr[i], self.indptr[i + 1])
        return self.indices[s], self.data[s]


def totals(L, comm):
    """Out_c, In_c, size_c indexed by community id, the members added in ascending order"""
    Out, In, size = np.zeros(L.m), np.zeros(L.m), np.zeros(L.m, dtype=np.int64)
    np.add.at(Out, comm, L.out)                    # (np.add.at adds one element after another, in index order)
    np.add.at(In, comm, L.inn)
    np.add.at(size, comm, 1)
    return Out, In, size


def scaled_modularity(L, comm, Out, In, w, gamma):
    internal = np.zeros(L.m)
    for i in range(L.m):
        cols, vals = L.row(i)
        acc = 0.0
        for v in vals[comm[cols] == comm[i]]:
            acc = acc + v
        internal[i] = acc
    return (w * 0.5) * ordered_sum(internal) - gamma * ordered_sum(Out * In)


def sweep(L, comm, Out, In, size, w, gamma):
    """every node's move against the snapshot (comm, Out, In, size): the new assignment and the number of nodes that moved"""
    new = comm.copy()
    moved = 0
    for i in range(L.m):
        cols, vals = L.row(i)
        keep = cols != i
        cols, vals = cols[keep], vals[keep]
        if cols.size == 0:
            continue
        X = comm[i]
        cs, inv = np.unique(comm[cols], return_inverse=True)
        k = np.zeros(cs.size)
        np.add.at(k, inv, vals)                    # per community, in the row's stored order
        at_x = np.flatnonzero(cs == X)
        kX = k[at_x[0]] if at_x.size else 0.0
        cand = cs != X
        if not cand.any():
            continue
        C, kC = cs[cand], k[cand]
        o, n_ = L.out[i], L.inn[i]
        g = w * (kC - kX) - gamma * (o * (In[C] - (In[X] - n_)) + n_ * (Out[C] - (Out[X] - o)))
        b = int(np.argmax(g))                      # the first maximum: the lowest C
        if g[b] > 0 and not (size[X] == 1 and size[C[b]] == 1 and C[b] > X):
            new[i] = C[b]
            moved += 1
    return new, moved


def run_level(L, w, gamma, tol, trace=None):
    """(kept assignment, its Out, In, size, Qs, sweeps run)"""
    comm = np.arange(L.m)
    Out, In, size = totals(L, comm)
    qs = scaled_modularity(L, comm, Out, In, w, gamma)
    if trace is not None:
        trace.append(qs)
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        new, moved = sweep(L, comm, Out, In, size, w, gamma)
        sweeps += 1
        if not moved:
            break
        nOut, nIn, nsize = totals(L, new)
        nqs = scaled_modularity(L, new, nOut, nIn, w, gamma)
        if not nqs - qs > tol * (w * w):
            break
        comm, Out, In, size, qs = new, nOut, nIn, nsize, nqs
        if trace is not None:
            trace.append(qs)
    return comm, Out, In, size, qs, sweeps


def aggregate(L, comm, Out, In, size):
    """(coarse level, coarse index of every node): ids ranked ascending; a coarse weight adds its fine edges in (row, column) order"""
    alive = np.flatnonzero(size > 0)
    rank = np.full(L.m, -1)
    rank[alive] = np.arange(alive.size)
    cn = rank[comm]
    acc = {}
    for u in range(L.m):
        cols, vals = L.row(u)
        for v, s in zip(cols, vals):
            key = (int(cn[u]), int(cn[v]))
            acc[key] = acc.get(key, 0.0) + s
    keys = sorted(acc)
    indptr = np.zeros(alive.size + 1, dtype=np.int64)
    for u, _ in keys:
        indptr[u + 1] += 1
    indptr = np.cumsum(indptr)
    indices = np.array([v for _, v in keys], dtype=np.int64)
    data = np.array([acc[k] for k in keys])
    return _Level(indptr, indices, data, Out[alive], In[alive]), cn


def renumber(labels):
    """0 .. k-1 by decreasing size, ties to the smallest member index"""
    labels = np.asarray(labels)
    ids, first, counts = np.unique(labels, return_index=True, return_counts=True)
    order = np.lexsort((first, -counts))
    new = np.empty(ids.size, dtype=np.int32)
    new[order] = np.arange(ids.size, dtype=np.int32)
    return new[np.searchsorted(ids, labels)]


def louvain(graph, resolution=1.0, tol=1e-3, max_levels=32, trace=None):
    """(labels int32, Q, (levels, sweeps, communities)) by the rule at the top.  ``trace``: a list that receives, per level, the list
    of the kept Qs values in order"""
    A = as_csr(graph)
    n = A.shape[0]
    out, inn, w = degrees(A)
    if n == 0 or w == 0:
        return np.arange(n, dtype=np.int32), 0.0, (0, 0, n)
    S = (A + A.T).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    L = _Level(S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data.copy(), out, inn)
    labels = np.arange(n)
    levels = sweeps = 0
    qs = 0.0
    while levels < max_levels:
        t = [] if trace is not None else None
        comm, Out, In, size, qs, s = run_level(L, w, resolution, tol, t)
        if trace is not None:
            trace.append(t)
        levels += 1
        sweeps += s
        coarse, cn = aggregate(L, comm, Out, In, size)
        labels = cn[labels]
        if coarse.m == L.m:
            break
        L = coarse
    labels = renumber(labels)
    return labels, qs / (w * w), (levels, sweeps, int(labels.max()) + 1)


# ---- the quality reference: classic sequential Louvain, nodes in index order, every move applied at once ----------------------------
def sequential_louvain(graph, resolution=1.0, max_levels=32):
    """(labels, Q): Blondel et al.'s local moving with the same directed gain, node after node in index order with the totals
    updated after every move, passes repeated until one moves nothing, then aggregation, until a level merges nothing"""
    A = as_csr(graph)
    n = A.shape[0]
    out, inn, w = degrees(A)
    if n == 0 or w == 0:
        return np.arange(n, dtype=np.int32), 0.0
    S = (A + A.T).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    L = _Level(S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data.copy(), out, inn)
    labels = np.arange(n)
    gamma = resolution
    for _ in range(max_levels):
        comm = np.arange(L.m)
        Out, In = L.out.copy(), L.inn.copy()
        for _pass in range(1000):
            moved = 0
            for i in range(L.m):
                cols, vals = L.row(i)
                keep = cols != i
                cols, vals = cols[keep], vals[keep]
                if cols.size == 0:
                    continue
                X = comm[i]
                cs, inv = np.unique(comm[cols], return_inverse=True)
                k = np.zeros(cs.size)
                np.add.at(k, inv, vals)
                at_x = np.flatnonzero(cs == X)
                kX = k[at_x[0]] if at_x.size else 0.0
                cand = cs != X
                if not cand.any():
                    continue
                C, kC = cs[cand], k[cand]
                o, n_ = L.out[i], L.inn[i]
                g = w * (kC - kX) - gamma * (o * (In[C] - (In[X] - n_)) + n_ * (Out[C] - (Out[X] - o)))
                b = int(np.argmax(g))
                if g[b] > 0:
                    Out[X] -= o
                    In[X] -= n_
                    Out[C[b]] += o
                    In[C[b]] += n_
                    comm[i] = C[b]
                    moved += 1
            if not moved:
                break
        Out, In, size = totals(L, comm)
        coarse, cn = aggregate(L, comm, Out, In, size)
        labels = cn[labels]
        if coarse.m == L.m:
            break
        L = coarse
    labels = renumber(labels)
    return labels, modularity(A, labels, gamma)
