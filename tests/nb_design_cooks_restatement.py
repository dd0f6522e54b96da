"""numpy statement of the Cook's-distance rule of DESIGN.md K28 (pilot_ot_nb_design_cooks) by ANOTHER ROUTE than the product's: the
cells from a dict of row bytes; np.sort and math.fsum where the device runs a bitonic network and a butterfly; the hat diagonal from
np.linalg.solve on the explicit X^T W X + lambda I, formed in np.longdouble and refined there (numpy's solvers take no long double:
the float64 solution is corrected with long-double residuals until it stops moving, which leaves an error of about cond * 2^-64, far
inside every tolerance the tests use), where the device inverts a Cholesky factor of per-lane partial sums.  Not collected by pytest
(no test_ prefix).  The gene classes of the GPU tests live here too, with the three conditions their comparisons rest on (no distance
next to the cutoff, no replacement next to an integer, a well-conditioned Gram matrix), checked HERE, on this restatement, when a
case is built."""
import functools
import math

import numpy as np

import nb_cooks_restatement as CR
import nb_design_restatement as DR
import nb_glm_restatement as RR

MIN_MU, RIDGE = DR.MIN_MU, DR.RIDGE
MIN_ROBUST_DISP, MIN_GROUP, MIN_REPLACE, BASE_TRIM = CR.MIN_ROBUST_DISP, CR.MIN_GROUP, CR.MIN_REPLACE, CR.BASE_TRIM
FALLBACK_TRIM, FALLBACK_SCALE = CR.Fraction(1, 8), 1.51
MAX_COND = 1e3
tm, cutoff, trim_rule, replacements, refit_max_cooks = CR.tm, CR.cutoff, CR.trim_rule, CR.replacements, CR.refit_max_cooks


def cells(X):
    """(codes int32, n_cells): samples with bit-identical rows share a cell; cells are numbered by first appearance"""
    seen = {}
    codes = np.array([seen.setdefault(np.ascontiguousarray(row, dtype=np.float64).tobytes(), len(seen)) for row in np.asarray(X)],
                     dtype=np.int32)
    return codes, len(seen)


def gram(w, X):
    """X^T diag(w) X + lambda I in long double"""
    Xl = np.asarray(X, dtype=np.longdouble)
    return (Xl * np.asarray(w, dtype=np.longdouble)[:, None]).T @ Xl + np.longdouble(RIDGE) * np.eye(X.shape[1], dtype=np.longdouble)


def solve_refined(M, B):
    """M^-1 B in long double: np.linalg.solve in float64, then residual corrections in long double until they stop mattering"""
    M64 = np.asarray(M, dtype=np.float64)
    B = np.asarray(B, dtype=np.longdouble)
    Z = np.linalg.solve(M64, np.asarray(B, dtype=np.float64)).astype(np.longdouble)
    for _ in range(8):
        R = B - M @ Z
        step = np.linalg.solve(M64, np.asarray(R, dtype=np.float64)).astype(np.longdouble)
        Z = Z + step
        if float(np.abs(step).max()) <= 1e-22 * float(np.abs(Z).max()):
            break
    return Z


def jacobi_cond(M):
    """cond_2 of D^-1/2 M D^-1/2, D = diag(M): the condition number the Cholesky solve's error bound carries"""
    M = np.asarray(M, dtype=np.float64)
    d = 1.0 / np.sqrt(np.diag(M))
    return float(np.linalg.cond(M * d[:, None] * d[None], 2))


def hat(w, X):
    """(h (m,), lambda tr(M^-1), kappa): h_j = w_j x_j^T M^-1 x_j with M = X^T W X + lambda I, as float64 rounded from long double"""
    M = gram(w, X)
    Xl = np.asarray(X, dtype=np.longdouble)
    Z = solve_refined(M, Xl.T)                                            # p x m: the columns M^-1 x_j
    h = np.asarray(w, dtype=np.longdouble) * (Xl * Z.T).sum(axis=1)
    trace = np.longdouble(RIDGE) * np.trace(solve_refined(M, np.eye(X.shape[1])))
    return np.asarray(h, dtype=np.float64), float(trace), jacobi_cond(M)


def robust_variance(q, codes, size):
    """K28's v: over the cells of 3 or more K25's per-group expression, else the 1/8-trimmed variance of all samples"""
    big = [g for g in range(size.size) if size[g] >= MIN_GROUP]
    if big:
        v = []
        for g in big:
            r, scale = trim_rule(size[g])
            x = q[codes == g]
            v.append(scale * tm((x - tm(x, r)) ** 2, r))
        return max(v)
    return FALLBACK_SCALE * tm((q - tm(q, FALLBACK_TRIM)) ** 2, FALLBACK_TRIM)


def cooks(counts, X, s, alpha, beta, cut, min_replace=MIN_REPLACE):
    """dict of per-gene arrays as engine.nb_design_cooks returns them, with D and H (m x G); D_scale: D with |c - mu| replaced by
    c + mu; kappa: the Jacobi-scaled cond_2 of the gene's M; ridge_trace: lambda tr(M^-1), so that sum_j h_j = p - ridge_trace"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    m, G = c.shape
    p = X.shape[1]
    codes, k = cells(X)
    size = np.bincount(codes, minlength=k)
    n_of = size[codes]
    elig = n_of >= MIN_GROUP
    out = {name: np.full(G, np.nan) for name in ("alpha_robust", "max_cooks", "trimmed_base", "kappa", "ridge_trace")}
    out["arg_max"] = np.full(G, -1, dtype=np.int32)
    out["n_above"], out["n_replace"] = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    D, H, scale_of = np.full((m, G), np.nan), np.full((m, G), np.nan), np.full((m, G), np.nan)
    for j in range(G):
        cj, a = c[:, j], alpha[j]
        if np.isnan(a) or not cj.any() or not np.isfinite(beta[j]).all():
            continue
        qj = cj / s
        out["trimmed_base"][j] = tm(qj, BASE_TRIM)
        mean_q = math.fsum(qj) / m
        a_rob = max((robust_variance(qj, codes, size) - mean_q) / mean_q ** 2, MIN_ROBUST_DISP)
        mu = np.maximum(s * np.exp(X @ beta[j]), MIN_MU)
        h, out["ridge_trace"][j], out["kappa"][j] = hat(mu / (1.0 + a * mu), X)
        tail = h / (p * (1.0 - h) ** 2) / (mu + a_rob * mu * mu)
        d, d_scale = (cj - mu) ** 2 * tail, (cj + mu) ** 2 * tail
        D[:, j], H[:, j], scale_of[:, j] = d, h, d_scale
        out["alpha_robust"][j] = a_rob
        if elig.any():
            top = d[elig].max()
            at = int(np.flatnonzero(elig & (d == top))[0])
            out["max_cooks"][j], out["arg_max"][j] = top, at
            out["n_above"][j] = np.count_nonzero(cj > cj[at])
        out["n_replace"][j] = np.count_nonzero((d > cut) & (n_of >= min_replace))
    out["D"], out["H"], out["D_scale"] = D, H, scale_of
    return out


# ---- the designs and the gene classes of the tests ------------------------------------------------------------------------------------
CLASSES = ("clean", "outlier in a replaceable cell", "outlier in a flaggable cell", "two outliers", "zeros", "nan dispersion")

# by their cell sizes (p = 2: [1, indicator]; p = 3: batch x group, the cells (b0 g0, b0 g1, b1 g0, b1 g1)), or numeric: (p, m)
CELL_DESIGNS = {2: [(3, 7), (2, 5), (23, 24), (32, 32), (64, 66)], 3: [(3, 7, 4, 6), (1, 3, 7, 2)]}
NUMERIC_DESIGNS = [(4, 24), (8, 9), (8, 65)]


def cell_design(rng, sizes):
    """X of the cell sizes in a shuffled sample order: two cells [1, group], four cells [1, batch, group]"""
    if len(sizes) == 2:
        rows = np.array([[1.0, 0.0], [1.0, 1.0]])
    elif len(sizes) == 4:
        rows = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0]])
    else:
        raise ValueError("two or four cells")
    return np.ascontiguousarray(rows[rng.permutation(np.repeat(np.arange(len(sizes)), sizes))])


def numeric_design(rng, p, m):
    """intercept, p - 2 covariates -- alternately a scaled age and a batch indicator, the age first so that every cell is one
    sample -- and the group last; full rank, cond_2 below 100 (so that the Gram matrix stays below MAX_COND for most genes)"""
    for _ in range(5000):
        cols = [np.ones(m)]
        for i in range(p - 2):
            if i % 2 == 0:
                a = rng.normal(0.0, 1.0, m)
                cols.append((a - a.mean()) / a.std(ddof=1))
            else:
                cols.append(rng.permutation(np.arange(m) % 2 == 1).astype(np.float64))
        cols.append(rng.permutation(np.arange(m) >= (m + 1) // 2).astype(np.float64))
        X = np.stack(cols, axis=1)
        if np.linalg.matrix_rank(X) == p and np.linalg.cond(X) < (100.0 if m > p + 1 else 1000.0):
            return np.ascontiguousarray(X)
    raise RuntimeError("no well-conditioned design of %d x %d found" % (m, p))


def _one_gene(rng, s, X, codes, size, kind):
    """(counts of one gene, its dispersion): K25's classes with the cells as the groups"""
    m = s.size
    base = float(np.exp(rng.uniform(np.log(20.0), np.log(3000.0))))
    coef = np.concatenate([[0.0], rng.normal(0.0, 0.3, X.shape[1] - 1)])
    c = RR.nb_counts(rng, (s * base * np.exp(X @ coef))[:, None], np.full((1, 1), 0.05 + 2.0 / base))[:, 0]
    alpha = float(np.clip(0.05 + 2.0 / max(c.mean(), 1.0), RR.MIN_DISP, RR.max_disp(m)))
    name = CLASSES[kind]

    def member(ok):
        pick = np.flatnonzero(ok) if ok.any() else np.arange(size.size)
        return int(rng.choice(np.flatnonzero(codes == rng.choice(pick))))

    if name.startswith("outlier") or name == "two outliers":
        c = np.maximum(c, 5.0)
        ok = (size >= MIN_GROUP) & (size < MIN_REPLACE) if name == "outlier in a flaggable cell" else size >= MIN_REPLACE
        hit = []
        while len(hit) < (2 if name == "two outliers" else 1):          # (two DIFFERENT samples: every count stays below 2^24)
            i = member(ok)
            if i not in hit:
                hit.append(i)
                c[i] = c[i] * 200.0
    elif name == "zeros":
        c = np.zeros(m)
    elif name == "nan dispersion":
        alpha = np.nan
    return c, alpha


def conditions_hold(want, s, cut, max_cond=MAX_COND):
    """per gene: K25's two conditions (nb_cooks_restatement.conditions_hold) and a Jacobi-scaled cond_2 of M of at most max_cond"""
    with np.errstate(invalid="ignore"):
        return CR.conditions_hold(want, s, cut) & ~(want["kappa"] > max_cond)


def case(seed, X, G, min_replace=MIN_REPLACE, max_cond=MAX_COND):
    """one test case on the design X: G genes cycling through the classes, their dispersions, the coefficients (K26's restatement;
    zeros where it fits none, so that the call's finite-beta check passes) and the restatement's answer.  A gene that breaks a
    condition is DROPPED, not drawn again: `generated` is how many were made, `kind` the classes of the kept ones."""
    rng = np.random.default_rng(seed)
    m, p = X.shape
    codes, k = cells(X)
    size = np.bincount(codes, minlength=k)
    s = CR.tied_size_factors(rng, m)
    cut = cutoff(m, p)
    kind = np.arange(G) % len(CLASSES)
    c, alpha = np.zeros((m, G)), np.zeros(G)
    for j in range(G):
        c[:, j], alpha[j] = _one_gene(rng, s, X, codes, size, kind[j])
    beta = DR.final_fit(c, X, s, alpha)[0]
    beta[np.isnan(beta).any(axis=1)] = 0.0
    want = cooks(c, X, s, alpha, beta, cut, min_replace)
    keep = np.flatnonzero(conditions_hold(want, s, cut, max_cond))
    c, alpha, beta, kind = np.ascontiguousarray(c[:, keep]), alpha[keep], np.ascontiguousarray(beta[keep]), kind[keep]
    want = {name: np.ascontiguousarray(v[..., keep]) for name, v in want.items()}
    out = dict(m=m, p=p, G=keep.size, generated=G, X=X, cells=codes, n_cells=k, sizes=size, s=s, c=c, alpha=alpha, beta=beta, cutoff=cut,
               kind=kind, want=want, min_replace=min_replace)
    for a in (X, codes, s, c, alpha, beta, kind) + tuple(want.values()):
        a.flags.writeable = False
    return out


def first_genes(C, G):
    """the case C cut to its first G genes (the classes cycle, so any six in a row hold one of each that was kept)"""
    out = dict(C, G=G, c=np.ascontiguousarray(C["c"][:, :G]), alpha=C["alpha"][:G], beta=np.ascontiguousarray(C["beta"][:G]), kind=C["kind"][:G])
    out["want"] = {name: np.ascontiguousarray(v[..., :G]) for name, v in C["want"].items()}
    return out


GENERATED = 72                                                             # genes made per design: twelve of every class


@functools.lru_cache(maxsize=None)
def design_case(key):
    """the one case of a design, built once and shared: key = ("cells", sizes) or ("numeric", p, m)"""
    if key[0] == "cells":
        sizes = key[1]
        X = cell_design(np.random.default_rng(100 * sum(sizes) + len(sizes)), sizes)
        return case(7 * sum(sizes) + len(sizes), X, GENERATED)
    _, p, m = key
    return case(7 * m + p, numeric_design(np.random.default_rng(100 * m + p), p, m), GENERATED)


DESIGN_KEYS = [("cells", sizes) for p in sorted(CELL_DESIGNS) for sizes in CELL_DESIGNS[p]] + [("numeric", p, m) for p, m in NUMERIC_DESIGNS]


def near_confounded_design(rng, m=16, eps=1e-4):
    """[1, batch, batch + eps * noise, group]: two columns that nearly coincide, so that the Jacobi-scaled cond_2 of M is about 1e8
    (the ridge keeps it from growing further); cond_2 of X itself stays far below the 1e8 the engine accepts"""
    batch = rng.permutation(np.arange(m) % 2 == 1).astype(np.float64)
    group = rng.permutation(np.arange(m) >= m // 2).astype(np.float64)
    return np.ascontiguousarray(np.stack([np.ones(m), batch, batch + eps * rng.normal(0.0, 1.0, m), group], axis=1))
