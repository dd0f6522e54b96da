"""Synchronous Leiden (K20) restated in numpy, the plain way, on top of tests/louvain_restatement.py: K17's move phase as it is, then
a refinement of its partition P under the same synchronous sweep, then K17's aggregation by the REFINED partition.  This file is
the rule the device is held to (pilot_amd/csrc/louvain_kernels.hpp states the same one); it is independent of the device code.

The rule.  Notation and sum orders are K17's (louvain_restatement's docstring); "stored neighbour" is a stored, non-zero entry
j != i.  A run is a sequence of levels; every level restarts from singletons.

  1. Move phase: LR.run_level, unchanged.  It gives P with totals OutP, InP.  If every community of P is one node the run ends: the
     level's nodes are the communities and Q = Qs(level start) / w^2.
  2. Refinement.  Fixed for the level, node i in X = P_i: e_i = sum of S_ij over stored neighbours with P_j = X, stored order;
         node_ok_i = [ w e_i - gamma (out_i (InP_X - in_i) + in_i (OutP_X - out_i)) >= 0 ]
     R starts as singletons; refinement sweeps use the move phase's loop (at most 128, kept iff Qs rises by more than tol w^2, ended
     by a sweep that moves nothing or is discarded).  Per snapshot (R, OutR, InR, sizeR): c_i = sum of S_ij over stored neighbours
     with P_j = P_i and R_j != R_i, stored order; cut_T = sum of c_i over T's members ascending;
         sub_ok_T = [ w cut_T - gamma (OutR_T (InP_X - InR_T) + InR_T (OutP_X - OutR_T)) >= 0 ],  X the P-community of T's members.
     Node i decides only if sizeR[R_i] = 1 and node_ok_i.  Candidates: the sub-communities T != R_i that hold a stored neighbour j
     with P_j = P_i and have sub_ok_T; k_T over those neighbours in stored order; g(T) is K17's g with X = R_i (so k_X = 0).
     Largest g, ties to the lowest T; the node moves iff g > 0 and not (sizeR_T = 1 and T > R_i).  Settle: a move into a T of size
     1 stands only if T's single member did not itself decide to leave (read from the unsettled decisions); `moved` counts the moves
     that stand.  Every product and sum is rounded on its own, in the order written.
  3. If R merged nothing the run ends as in 1.  Else aggregate by R (LR.aggregate); after level max_levels the run ends there, the
     coarse nodes are the communities and Q = Qs(R kept) / w^2; otherwise the next level runs on the coarse graph.
  4. Labels: LR.renumber.

Every returned community is connected in S: only singletons move, a community of two or more never loses a member during the
refinement, a joiner has an edge to a member that stays, and level nodes are connected sets joined only along edges."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from louvain_restatement import (MAX_SWEEPS, _Level, aggregate, as_csr, degrees, modularity, renumber, run_level,  # noqa: F401
                                 scaled_modularity, totals)


def _inside(L, i, P):
    """(columns, weights) of row i's stored neighbours j != i in i's community of P, in stored order"""
    cols, vals = L.row(i)
    keep = (cols != i) & (P[cols] == P[i])
    return cols[keep], vals[keep]


def _ordered(vals):
    acc = 0.0
    for v in vals:
        acc = acc + float(v)
    return acc


def node_ok(L, P, OutP, InP, w, gamma):
    ok = np.zeros(L.m, dtype=bool)
    for i in range(L.m):
        e = _ordered(_inside(L, i, P)[1])
        X, o, n_ = P[i], L.out[i], L.inn[i]
        ok[i] = w * e - gamma * (o * (InP[X] - n_) + n_ * (OutP[X] - o)) >= 0
    return ok


def sub_ok(L, P, OutP, InP, R, Out, In, w, gamma):
    """indexed by sub-community id; False where the id has no member"""
    c = np.zeros(L.m)
    for i in range(L.m):
        cols, vals = _inside(L, i, P)
        c[i] = _ordered(vals[R[cols] != R[i]])
    cut = np.zeros(L.m)
    np.add.at(cut, R, c)                           # members ascending
    ok = np.zeros(L.m, dtype=bool)
    for i in range(L.m):
        T, X = R[i], P[i]
        ok[T] = w * cut[T] - gamma * (Out[T] * (InP[X] - In[T]) + In[T] * (OutP[X] - Out[T])) >= 0
    return ok


def refine_sweep(L, P, OutP, InP, nok, R, Out, In, size, w, gamma):
    """(new assignment, moves that stand, the nodes that decided, the nodes that moved, moves the settle step cancelled)"""
    sok = sub_ok(L, P, OutP, InP, R, Out, In, w, gamma)
    raw = R.copy()
    decided = []
    for i in range(L.m):
        X = R[i]
        if size[X] != 1 or not nok[i]:
            continue
        decided.append(i)
        cols, vals = _inside(L, i, P)
        if cols.size == 0:
            continue
        cs, inv = np.unique(R[cols], return_inverse=True)
        k = np.zeros(cs.size)
        np.add.at(k, inv, vals)                    # per sub-community, in the row's stored order
        cand = sok[cs] & (cs != X)
        if not cand.any():
            continue
        T, kT = cs[cand], k[cand]
        o, n_ = L.out[i], L.inn[i]
        g = w * (kT - 0.0) - gamma * (o * (In[T] - (In[X] - n_)) + n_ * (Out[T] - (Out[X] - o)))
        b = int(np.argmax(g))
        if g[b] > 0 and not (size[T[b]] == 1 and T[b] > X):
            raw[i] = T[b]
    owner = np.full(L.m, -1)
    for i in range(L.m):
        if size[R[i]] == 1:
            owner[R[i]] = i
    new = raw.copy()
    cancelled = 0
    for i in range(L.m):
        T = raw[i]
        if T != R[i] and size[T] == 1 and raw[owner[T]] != R[owner[T]]:
            new[i] = R[i]
            cancelled += 1
    movers = np.flatnonzero(new != R)
    return new, movers.size, np.array(decided, dtype=np.int64), movers, cancelled


def refine(L, P, OutP, InP, w, gamma, tol, level=0, trace=None):
    """(kept refinement, its Out, In, size, Qs, sweeps run)"""
    nok = node_ok(L, P, OutP, InP, w, gamma)
    R = np.arange(L.m)
    Out, In, size = totals(L, R)
    qs = scaled_modularity(L, R, Out, In, w, gamma)
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        new, moved, decided, movers, cancelled = refine_sweep(L, P, OutP, InP, nok, R, Out, In, size, w, gamma)
        sweeps += 1
        if trace is not None:
            trace.append({"level": level, "decided": decided.size, "cancelled": cancelled, "moved": moved, "decided_nodes": decided,
                          "moved_nodes": movers, "degree": np.diff(L.indptr)})
        if not moved:
            break
        nOut, nIn, nsize = totals(L, new)
        nqs = scaled_modularity(L, new, nOut, nIn, w, gamma)
        if not nqs - qs > tol * (w * w):
            break
        R, Out, In, size, qs = new, nOut, nIn, nsize, nqs
    return R, Out, In, size, qs, sweeps


def leiden(graph, resolution=1.0, tol=1e-3, max_levels=32, trace=None):
    """(labels int32, Q, (levels, move sweeps, refinement sweeps, communities)) by the rule at the top.  ``trace``: a list that
    receives one dict per refinement sweep: ``level``, ``decided`` (nodes that decided), ``cancelled`` (moves the settle step
    cancelled), ``moved`` (moves that stand), and, for the tests of the degree bins, ``decided_nodes``, ``moved_nodes`` and the
    level's ``degree`` array"""
    A = as_csr(graph)
    n = A.shape[0]
    out, inn, w = degrees(A)
    if n == 0 or w == 0:
        return np.arange(n, dtype=np.int32), 0.0, (0, 0, 0, n)
    S = (A + A.T).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    L = _Level(S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data.copy(), out, inn)
    labels = np.arange(n)
    levels = move_sweeps = refine_sweeps = 0
    while True:
        start = []
        P, OutP, InP, sizeP, _, s = run_level(L, w, resolution, tol, start)
        qs = start[0]                              # Qs of the level's singletons
        levels += 1
        move_sweeps += s
        if (sizeP > 0).sum() == L.m:
            break
        R, Out, In, size, qs_r, s = refine(L, P, OutP, InP, w, resolution, tol, levels - 1, trace)
        refine_sweeps += s
        coarse, cn = aggregate(L, R, Out, In, size)
        if coarse.m == L.m:
            break
        labels = cn[labels]
        qs = qs_r
        if levels == max_levels:
            break
        L = coarse
    labels = renumber(labels)
    return labels, qs / (w * w), (levels, move_sweeps, refine_sweeps, int(labels.max()) + 1)


def disconnected(graph, labels):
    """the number of communities whose members are not connected in S = A + A^T"""
    A = as_csr(graph)
    S = (A + A.T).tocsr()
    labels = np.asarray(labels)
    bad = 0
    for c in np.unique(labels):
        members = np.flatnonzero(labels == c)
        if members.size > 1 and connected_components(S[members][:, members], directed=False)[0] > 1:
            bad += 1
    return bad
