"""The negative-binomial GLM for a general design (K26) restated in numpy / scipy, vectorised over genes x grid points.
Shared by test_nb_design_args.py, which pins these functions to scipy on their own, and test_gpu_nb_design.py, which holds the device
to them.  Nothing here imports the product.

Layout: c is samples x genes (rint of the counts), X the m x p design (first column ones), s the size factors; alpha or
x = log(alpha) is one value per gene (G,) or a row of values per gene (G, T); beta is (G, p) or (G, T, p)."""
import numpy as np
from scipy import special, stats

import nb_glm_restatement as R

MIN_DISP, MIN_MU, RIDGE, TOL, MAX_STEPS, MAX_HALVINGS = R.MIN_DISP, R.MIN_MU, 1e-6, 1e-10, 100, 30
max_disp, size_factors, nb_counts, grid_search = R.max_disp, R.size_factors, R.nb_counts, R.grid_search


# ---- step 2: the inner fit ---------------------------------------------------------------------------------------------------------
def penalised_loglik(c, X, s, alpha, beta):
    """l_lambda(beta) of one gene: c (m,), beta (p,)"""
    mu = s * np.exp(X @ beta)
    r = 1.0 / alpha
    return float(stats.nbinom.logpmf(c, r, r / (r + mu)).sum() - 0.5 * RIDGE * (beta ** 2).sum())


def weighted_gram(w, X):
    """(N, p, p): X^T diag(w_n) X for the weights w (m, N)"""
    return np.swapaxes(w.T[:, :, None] * X[None], 1, 2) @ X


def newton_step(c, X, s, alpha, beta):
    """the Newton step of l_lambda at beta, for N problems: c (m, N), alpha (N,), beta (N, p) -> (N, p).  Observed information
    sum_j w_j x_j x_j^T + lambda I with w = mu (1 + alpha c) / (1 + alpha mu)^2; score X^T (c - mu) / (1 + alpha mu) - lambda beta."""
    p = X.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        mu = np.exp(X @ beta.T + np.log(s)[:, None])
        inv = 1.0 / (1.0 + alpha[None] * mu)
        r = (c - mu) * inv
        w = (mu * inv) * ((1.0 + alpha[None] * c) * inv)
        H = weighted_gram(w, X) + RIDGE * np.eye(p)[None]
        g = (X.T @ r).T - RIDGE * beta
        bad = ~(np.isfinite(H).all(axis=(1, 2)) & np.isfinite(g).all(axis=1))
        H[bad], g[bad] = np.eye(p), np.nan
        return np.linalg.solve(H, g[:, :, None])[:, :, 0]


def cold_start(c, s, p):
    """(N, p): (log max(mean c / s, minmu), 0, ...)"""
    beta = np.zeros((c.shape[1], p))
    beta[:, 0] = np.log(np.maximum((c / s[:, None]).mean(axis=0), MIN_MU))
    return beta


def fit(c, X, s, alpha, start=None):
    """the maximiser of l_lambda for N problems: c (m, N), alpha (N,) -> (beta (N, p), steps (N,), converged (N,)).  Newton steps,
    halved while l_lambda would fall (the change summed term by term), until max |step| <= 1e-10; at most 100."""
    m, N = c.shape
    beta = cold_start(c, s, X.shape[1]) if start is None else np.array(start, dtype=np.float64)
    steps, conv = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool)
    act, ls = np.arange(N), np.log(s)
    for _ in range(MAX_STEPS):
        if act.size == 0:
            break
        b, a, cc = beta[act], alpha[act], c[:, act]
        d = newton_step(cc, X, s, a, b)
        moved = np.abs(d).max(axis=1)
        with np.errstate(over="ignore", invalid="ignore"):
            amu = a[None] * np.exp(X @ b.T + ls[:, None])
            rho, Xd = amu / (1.0 + amu), X @ d.T
            t, need = np.ones(act.size), ~(moved <= TOL)
            for _ in range(MAX_HALVINGS):
                if not need.any():
                    break
                D, td = t[None] * Xd, t[:, None] * d
                change = (cc * D - (cc + 1.0 / a[None]) * np.log1p(rho * np.expm1(D))).sum(axis=0) - 0.5 * RIDGE * (td * (2 * b + td)).sum(axis=1)
                need &= ~(np.isfinite(change) & (change >= 0))
                t = np.where(need, 0.5 * t, t)
            beta[act] = b + t[:, None] * d
            done = t * moved <= TOL
        steps[act] += 1
        conv[act[done]] = True
        act = act[~done]
    return beta, steps, conv


def fit_grid(c, X, s, x):
    """beta^(alpha) at every x of the (G, T) grid: (G, T, p), and whether every fit converged"""
    G, T = x.shape
    beta, _, conv = fit(np.repeat(c, T, axis=1), X, s, np.exp(x).ravel())
    return beta.reshape(G, T, -1), bool(conv.all())


# ---- step 3: the adjusted profile likelihood ---------------------------------------------------------------------------------------
def floored_mu(X, s, beta):
    """(m, G, T): max(s_j exp(x_j^T beta), minmu) for beta (G, T, p)"""
    with np.errstate(over="ignore"):
        return np.maximum(s[:, None, None] * np.exp(np.einsum("jk,gtk->jgt", X, beta)), MIN_MU)


def likelihood_terms(c, mu, x):
    """the four terms of the bracket of L, each (m, G, T), for mu (m, G, T) and x (G, T)"""
    alpha = np.exp(x)[None]
    r, am, cc = 1.0 / alpha, alpha * mu, c[:, :, None]
    return special.gammaln(cc + r), -special.gammaln(r) + 0.0 * cc, -(cc + r) * np.log1p(am), np.where(cc > 0, cc * np.log(am), 0.0)


def objective_at(c, X, s, x, beta, log_prior_mean=None, prior_var=None):
    """L(x) (G, T) with the coefficients beta (G, T, p) given: the likelihood at the floored means minus 1/2 log det X^T W X"""
    mu = floored_mu(X, s, beta)
    w = mu / (1.0 + np.exp(x)[None] * mu)
    logdet = np.linalg.slogdet(weighted_gram(w.reshape(w.shape[0], -1), X))[1].reshape(x.shape)
    L = sum(t.sum(axis=0) for t in likelihood_terms(c, mu, x)) - 0.5 * logdet
    if log_prior_mean is not None:
        L = L - (x - np.asarray(log_prior_mean)[:, None]) ** 2 / (2.0 * prior_var)
    return L


def objective(c, X, s, x, log_prior_mean=None, prior_var=None):
    """L(x), beta re-solved at every x; the shape of x, (G,) or (G, T)"""
    x = np.asarray(x, dtype=np.float64)
    xg = x[:, None] if x.ndim == 1 else x
    L = objective_at(c, X, s, xg, fit_grid(c, X, s, xg)[0], log_prior_mean, prior_var)
    return L[:, 0] if x.ndim == 1 else L


def bound(c, X, s, x):
    """B of the parity rule at x (G,): K22's with k -> p^2 for the determinant: 64 ulp of the magnitudes actually added"""
    m, p = X.shape
    xg = x[:, None]
    mu = floored_mu(X, s, fit_grid(c, X, s, xg)[0])
    mag = sum(np.abs(t).sum(axis=0) for t in likelihood_terms(c, mu, xg))[:, 0]
    return 64 * 2.0 ** -53 * (mag + 4 * m + p * p)


def dispersions(counts, X, s, log_prior_mean=None, prior_var=None, chunk=64):
    """(x, L(x)) per gene by the six rounds of the 64-point grid; NaN for a gene of zeros"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    m, G = c.shape
    x, L = np.full(G, np.nan), np.full(G, np.nan)
    live = np.flatnonzero((c > 0).any(axis=0))
    for a in range(0, live.size, chunk):
        j = live[a:a + chunk]
        prior = None if log_prior_mean is None else np.asarray(log_prior_mean)[j]
        start = [None]

        def f(xs, j=j, prior=prior, start=start):
            # (the fits of a round start from the coefficients at the round before's maximum: the optimum does not depend on the
            # start, the time does)
            T = xs.shape[1]
            first = None if start[0] is None else np.repeat(start[0], T, axis=0)
            beta = fit(np.repeat(c[:, j], T, axis=1), X, s, np.exp(xs).ravel(), first)[0].reshape(j.size, T, -1)
            Lx = objective_at(c[:, j], X, s, xs, beta, prior, prior_var)
            start[0] = beta[np.arange(j.size), np.argmax(Lx, axis=1)]
            return Lx

        x[j], L[j] = grid_search(f, np.full(j.size, np.log(MIN_DISP)), np.full(j.size, np.log(max_disp(m))))
    return x, L


def resolved(c, X, s, x, delta=1e-4, log_prior_mean=None, prior_var=None):
    """the genes whose maximiser is pinned: interior, and L drops by more than 2 B at x -+ delta"""
    m = c.shape[0]
    out = np.zeros(x.size, dtype=bool)
    j = np.flatnonzero(np.isfinite(x))
    if j.size == 0:
        return out
    cj, xj = c[:, j], x[j]
    prior = None if log_prior_mean is None else np.asarray(log_prior_mean)[j]
    L = objective(cj, X, s, np.stack([xj - delta, xj, xj + delta], axis=1), prior, prior_var)
    B = bound(cj, X, s, xj)
    interior = (xj - delta > np.log(MIN_DISP)) & (xj + delta < np.log(max_disp(m)))
    out[j] = interior & (L[:, 1] - L[:, 0] > 2 * B) & (L[:, 1] - L[:, 2] > 2 * B)
    return out


# ---- step 5: the final fit ---------------------------------------------------------------------------------------------------------
def fit_outputs(c, X, s, alpha, beta):
    """(Sigma (G, p, p), loglik (G,), its bound (G,)) at given coefficients beta (G, p): Sigma = (X^T W X + lambda I)^-1 with W at the
    floored means; loglik = sum_j nbinom.logpmf(c_j; mu_j, alpha) at the unfloored ones, within 64 ulp of the magnitudes added"""
    m, p = X.shape
    mu = s[:, None] * np.exp(X @ beta.T)
    fl = np.maximum(mu, MIN_MU)
    w = fl / (1.0 + alpha[None] * fl)
    cov = np.linalg.inv(weighted_gram(w, X) + RIDGE * np.eye(p)[None])
    r = 1.0 / alpha[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = (special.gammaln(c + r), -special.gammaln(r) + 0.0 * c, -special.gammaln(c + 1.0), -(c + r) * np.log1p(alpha[None] * mu),
                 np.where(c > 0, c * np.log(alpha[None] * mu), 0.0))
    loglik = sum(t.sum(axis=0) for t in terms)
    return cov, loglik, 64 * 2.0 ** -53 * (sum(np.abs(t).sum(axis=0) for t in terms) + 5 * m)


def final_fit(counts, X, s, alpha):
    """(beta, Sigma, loglik) per gene at the dispersions alpha; NaN for a NaN alpha or a gene of zeros"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    G, p = c.shape[1], X.shape[1]
    alpha = np.asarray(alpha, dtype=np.float64)
    beta, cov, loglik = np.full((G, p), np.nan), np.full((G, p, p), np.nan), np.full(G, np.nan)
    j = np.flatnonzero(~np.isnan(alpha) & (c > 0).any(axis=0))
    if j.size:
        beta[j] = fit(c[:, j], X, s, alpha[j])[0]
        cov[j], loglik[j], _ = fit_outputs(c[:, j], X, s, alpha[j], beta[j])
    return beta, cov, loglik


# ---- step 6: the host tail ---------------------------------------------------------------------------------------------------------
def wald(beta, cov, contrast):
    """(log2 fold change, its standard error, the statistic, the two-sided p-value) of the contrast a"""
    a = np.asarray(contrast, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lfc = np.log2(np.e) * (beta @ a)
        se = np.log2(np.e) * np.sqrt(np.einsum("k,gkl,l->g", a, cov, a))
        stat = lfc / se
    return lfc, se, stat, 2.0 * stats.norm.sf(np.abs(stat))


def lrt(loglik_full, loglik_reduced):
    """(statistic, p-value) of the likelihood-ratio test with one degree of freedom"""
    stat = 2.0 * (loglik_full - loglik_reduced)
    return stat, stats.chi2.sf(stat, 1)


# ---- the designs and gene classes of the tests ---------------------------------------------------------------------------------------
def make_design(rng, m, p):
    """(X, kinds): the intercept, p - 2 covariate columns -- alternately a batch indicator and an age scaled to unit ddof-1
    standard deviation -- and the group indicator last; full rank, condition number below 1e3"""
    kinds = ["intercept"] + [("batch", "age")[i % 2] for i in range(p - 2)] + ["group"]
    for _ in range(1000):
        cols = []
        for kind in kinds:
            if kind == "intercept":
                cols.append(np.ones(m))
            elif kind == "age":
                a = rng.normal(0.0, 1.0, m)
                cols.append((a - a.mean()) / a.std(ddof=1))
            else:
                cols.append(rng.permutation((np.arange(m) % 2 == 1) if kind == "batch" else (np.arange(m) >= (m + 1) // 2)).astype(np.float64))
        X = np.stack(cols, axis=1)
        if np.linalg.matrix_rank(X) == p and np.linalg.cond(X) < 1e3:
            return X, kinds
    raise RuntimeError("no full-rank design of %d x %d found" % (m, p))


def planted(rng, kinds, G):
    """(p, G) coefficients without the intercept's: batch N(0, 0.5), scaled age N(0, 0.3), a group effect N(0, 1) on 30 % of the genes"""
    rows = []
    for kind in kinds:
        if kind == "batch":
            rows.append(rng.normal(0.0, 0.5, G))
        elif kind == "age":
            rows.append(rng.normal(0.0, 0.3, G))
        elif kind == "group":
            rows.append(np.where(rng.random(G) < 0.3, rng.normal(0.0, 1.0, G), 0.0))
        else:
            rows.append(np.zeros(G))
    return np.stack(rows)


def nb_class(rng, s, X, kinds, G):
    """the NB generator of nb_glm_restatement with planted coefficients: base mean log-uniform on [2, 3000], alpha = 0.05 + 2 / base"""
    base = np.exp(rng.uniform(np.log(2.0), np.log(3000.0), G))
    mean = s[:, None] * base[None] * np.exp(X @ planted(rng, kinds, G))
    return nb_counts(rng, mean, (0.05 + 2.0 / base)[None])
