"""The elastic principal tree (Albergante et al., Entropy 2020) as this library states it (README, "Principal tree"),
in plain numpy, with the margin of every discrete decision it takes.  Nothing here calls the library.

A tree on m nodes has the spring matrix S = sum over edges of lam v v^T (v = e_a - e_b) + sum over nodes c of degree k >= 2 of
mu s s^T (s = e_c - (1 / k) sum of e_l over c's neighbours).  A fit repeats at most max_iter times: every point to the node of
smallest squared distance (float64 direct differences between the stored values and the nodes ROUNDED TO X's dtype; ties to the
lowest node), cnt / sum per node (np.add.at), (diag(cnt) / n + S) Y' = sum / n (numpy.linalg.solve),
change = max_j |Y'_j - Y_j| / |Y'_j - c|, Y <- Y', stop once change < eps.  One more partition of the final Y gives cnt, sum and
MSE = mean |x_i - y_a(i)|^2 against the unrounded nodes; E = MSE + trace(Y^T S Y).

The tree starts as c -/+ sqrt(w) v (leading eigenpair of the covariance, v's largest entry positive), is fitted, and grows by
grow, grow, shrink until it has M nodes; the winner of a step is the lowest-listed candidate with E <= E_min (1 + 1e-10).
Pseudotime: every point onto its nearest edge (float64 distance to the clipped projection, ties to the lowest edge)."""
import numpy as np

BAND = 1e-10


class Margins:
    """the smallest distance of every kind of decision from its edge, over everything computed since it was made"""

    def __init__(self):
        self.partition, self.stop, self.projection = np.inf, np.inf, np.inf
        self.band_in, self.band_out = 0.0, np.inf
        self.cond = 1.0


def springs(m, edges, lam=0.01, mu=0.1):
    S = np.zeros((m, m))
    nb = [[] for _ in range(m)]
    for a, b in edges:
        v = np.zeros(m); v[a], v[b] = 1.0, -1.0
        S += lam * np.outer(v, v)
        nb[a].append(b); nb[b].append(a)
    for c in range(m):
        if len(nb[c]) >= 2:
            s = np.zeros(m); s[c] = 1.0
            for l in nb[c]:
                s[l] -= 1.0 / len(nb[c])
            S += mu * np.outer(s, s)
    return S


def partition(X, Y, margins=None):
    """(assignment, cnt, sum, MSE) of the points X (n x D, any float dtype) for the nodes Y (m x D float64)"""
    Xd = X.astype(np.float64)
    Yt = Y.astype(X.dtype).astype(np.float64)
    d = ((Xd[:, None, :] - Yt[None, :, :]) ** 2).sum(axis=2)
    a = np.argmin(d, axis=1)
    if margins is not None:
        two = np.sort(d, axis=1)[:, :2]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
        margins.partition = min(margins.partition, float(gap.min()))
    m = Y.shape[0]
    cnt = np.zeros(m, dtype=np.int64)
    s = np.zeros_like(Y)
    np.add.at(cnt, a, 1)
    np.add.at(s, a, Xd)
    mse = float(((Xd - Y[a]) ** 2).sum(axis=1).sum() / X.shape[0])
    return a, cnt, s, mse


def elastic(Y, S):
    return float(np.trace(Y.T @ S @ Y))


def fit(X, Y0, S, centre, max_iter=10, eps=0.01, margins=None):
    """One candidate.  Returns a dict: nodes, mse, elastic, energy, iters, converged, singular, counts, sums, conds (one per solved
    system) and trace (the energy MSE + elastic at every partition, the final one included)."""
    n = X.shape[0]
    Y = np.array(Y0, dtype=np.float64)
    out = {"iters": 0, "converged": False, "singular": False, "conds": [], "trace": []}
    for _ in range(max_iter):
        _, cnt, s, mse = partition(X, Y, margins)
        out["trace"].append(mse + elastic(Y, S))
        A = np.diag(cnt / n) + S
        try:
            Ynew = np.linalg.solve(A, s / n)
        except np.linalg.LinAlgError:
            out["singular"] = True
            break
        out["conds"].append(float(np.linalg.cond(A)))
        num = np.sqrt(((Ynew - Y) ** 2).sum(axis=1))
        den = np.sqrt(((Ynew - centre) ** 2).sum(axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            change = float(np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0)).max())
        Y = Ynew
        out["iters"] += 1
        if margins is not None:
            margins.stop = min(margins.stop, abs(change - eps) / eps if eps > 0 else np.inf)
            margins.cond = max(margins.cond, out["conds"][-1])
        if change < eps:
            out["converged"] = True
            break
    _, cnt, s, mse = partition(X, Y, margins)
    out.update(nodes=Y, counts=cnt, sums=s, mse=mse, elastic=elastic(Y, S))
    out["energy"] = np.nan if out["singular"] else mse + out["elastic"]
    out["trace"].append(out["energy"])
    return out


def _neighbours(m, edges):
    nb = [[] for _ in range(m)]
    for a, b in edges:
        nb[a].append(b); nb[b].append(a)
    return nb


def _renumber(edges, gone, into=None):
    res = []
    for e in edges:
        e = [into if (v == gone and into is not None) else v for v in e]
        res.append(tuple(v - 1 if v > gone else v for v in e))
    return res


def grow(Y, edges, cnt, s):
    m = Y.shape[0]
    nb = _neighbours(m, edges)
    cands = []
    for i, (a, b) in enumerate(edges):
        e = list(edges); e[i] = (a, m); e.append((m, b))
        cands.append((np.vstack([Y, (Y[a] + Y[b]) / 2]), e))
    for v in range(m):
        if len(nb[v]) == 1:
            y = 2 * Y[v] - Y[nb[v][0]]
        elif cnt[v] > 0:
            y = s[v] / cnt[v]
        else:
            y = Y[nb[v]].mean(axis=0)
        cands.append((np.vstack([Y, y]), list(edges) + [(v, m)]))
    return cands


def shrink(Y, edges):
    m = Y.shape[0]
    nb = _neighbours(m, edges)
    cands = []
    for i, (a, b) in enumerate(edges):
        keep, gone = min(a, b), max(a, b)
        Z = Y.copy(); Z[keep] = (Y[a] + Y[b]) / 2
        cands.append((np.delete(Z, gone, axis=0), _renumber(edges[:i] + edges[i + 1:], gone, keep)))
    for v in range(m):
        if len(nb[v]) == 1:
            cands.append((np.delete(Y, v, axis=0), _renumber([e for e in edges if v not in e], v)))
    return cands


def start(X):
    Xd = X.astype(np.float64)
    c = Xd.mean(axis=0)
    w, V = np.linalg.eigh((Xd - c).T @ (Xd - c) / (X.shape[0] - 1))
    w, v = w[-1], V[:, -1]
    if not w > 0:
        raise ValueError("all points coincide")
    if v[np.argmax(np.abs(v))] < 0:
        v = -v
    return c, np.stack([c - np.sqrt(w) * v, c + np.sqrt(w) * v])


def tree(X, M, lam=0.01, mu=0.1, max_iter=10, eps=0.01):
    """Returns (nodes, edges, info): info holds winners, candidates and energy per step (step 0: the start) and the Margins."""
    mg = Margins()
    c, Y = start(X)
    edges = [(0, 1)]
    info = {"winners": [], "candidates": [], "energy": [], "margins": mg}

    def step(cands):
        fits = [fit(X, Yc, springs(Yc.shape[0], ec, lam, mu), c, max_iter, eps, mg) for Yc, ec in cands]
        for k, f in enumerate(fits):
            if f["singular"]:
                raise ValueError("candidate %d is singular" % k)
        E = np.array([f["energy"] for f in fits])
        gaps = (E - E.min()) / E.min()
        tied = gaps <= BAND
        mg.band_in = max(mg.band_in, float(gaps[tied].max()))
        if (~tied).any():
            mg.band_out = min(mg.band_out, float(gaps[~tied].min()))
        win = int(np.flatnonzero(tied)[0])
        info["winners"].append(win); info["candidates"].append(len(cands)); info["energy"].append(float(E[win]))
        return fits[win]["nodes"], cands[win][1], fits[win]["counts"], fits[win]["sums"]

    Y, edges, cnt, s = step([(Y, edges)])
    while Y.shape[0] < M:
        for kind in ("grow", "grow", "shrink"):
            Y, edges, cnt, s = step(grow(Y, edges, cnt, s) if kind == "grow" else shrink(Y, edges))
    return Y, np.array(edges, dtype=np.int64).reshape(-1, 2), info


def energy_of(X, Y, edges, lam=0.01, mu=0.1):
    """MSE + elastic energy of the tree as it stands (one partition, no fit)"""
    _, _, _, mse = partition(X, Y)
    return mse + elastic(Y, springs(Y.shape[0], [tuple(e) for e in edges], lam, mu))


def orient(Y, edges, source):
    """(edges as (a, b) with a nearer the source, in the order given; the tree distance from the source to every node)"""
    m = Y.shape[0]
    base = np.full(m, np.nan); base[source] = 0.0
    out = [tuple(int(v) for v in e) for e in edges]
    todo = [int(source)]
    while todo:
        a = todo.pop()
        for k, (p, q) in enumerate(list(out)):
            for u, v in ((p, q), (q, p)):
                if u == a and np.isnan(base[v]):
                    base[v] = base[a] + np.linalg.norm(Y[v] - Y[a]); out[k] = (u, v); todo.append(v)
    return np.array(out, dtype=np.int64), base


def project(X, Y, edges, source=0, margins=None):
    """Returns (pseudotime, d2, edge, t, projected points)"""
    Xd = X.astype(np.float64)
    E, base = orient(Y, edges, source)
    A, Bv = Y[E[:, 0]], Y[E[:, 1]] - Y[E[:, 0]]
    L2 = (Bv ** 2).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(L2 > 0, ((Xd[:, None, :] - A[None]) * Bv[None]).sum(axis=2) / L2, 0.0)
    t = np.clip(t, 0.0, 1.0)
    P = A[None] + t[:, :, None] * Bv[None]
    d2 = ((Xd[:, None, :] - P) ** 2).sum(axis=2)
    e = np.argmin(d2, axis=1)
    rows = np.arange(X.shape[0])
    if margins is not None:
        scale = 1e-9 * np.abs(Xd - Xd.mean(axis=0)).max()
        other = np.abs(P - P[rows, e][:, None, :]).max(axis=2) > scale
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.where(other, (d2 - d2[rows, e][:, None]) / d2, np.inf)
        margins.projection = min(margins.projection, float(gap.min()))
    te = t[rows, e]
    return base[E[e, 0]] + te * np.sqrt(L2[e]), d2[rows, e], e, te, P[rows, e]


def is_tree(m, edges):
    edges = [tuple(int(v) for v in e) for e in edges]
    if len(edges) != m - 1:
        return False
    seen, todo = {0}, [0]
    nb = _neighbours(m, edges)
    while todo:
        for v in nb[todo.pop()]:
            if v not in seen:
                seen.add(v); todo.append(v)
    return len(seen) == m
