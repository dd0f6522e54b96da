"""The negative-binomial GLM for a one-factor design (K22) restated in numpy / scipy, vectorised over genes x grid points
(a Python loop per gene takes 13 ms a gene).  Shared by test_nb_glm_args.py, which pins these functions to scipy on their own, and
test_gpu_nb_glm.py, which holds the device to them.  Nothing here imports the product.

Layout: c is samples x genes (rint of the counts), codes one group per sample, s the size factors; x = log(alpha) is one value per
gene (G,) or a row of values per gene (G, P)."""
import numpy as np
from scipy import special, stats

MIN_DISP, MIN_MU, GRID, ROUNDS = 1e-8, 0.5, 64, 6
NOT_CONVERGED, FLOORED = 1, 2


def max_disp(m):
    return float(max(10, m))


def group_means(c, codes, k, s):
    """(G, k): per gene and group the mean of c / s"""
    q = c / s[:, None]
    return np.stack([q[codes == g].mean(axis=0) for g in range(k)], axis=1)


def fitted_mu(c, codes, k, s):
    """(m, G): mu_j = max(s_j * the mean of c / s over j's group, minmu)"""
    return np.maximum(s[:, None] * group_means(c, codes, k, s).T[codes], MIN_MU)


def _as_grid(x):
    x = np.asarray(x, dtype=np.float64)
    return (x[:, None], True) if x.ndim == 1 else (x, False)


def likelihood_terms(c, mu, x):
    """the four terms of the bracket of L, each of shape (m, G, P): lgamma(c + r), -lgamma(r), -(c + r) log1p(a mu), c log(a mu)"""
    x, _ = _as_grid(x)
    alpha = np.exp(x)[None]
    r = 1.0 / alpha
    am = alpha * mu[:, :, None]
    cc = c[:, :, None]
    return special.gammaln(cc + r), -special.gammaln(r) + 0.0 * cc, -(cc + r) * np.log1p(am), np.where(cc > 0, cc * np.log(am), 0.0)


def cox_reid(mu, codes, k, x):
    """(G, P): sum over the groups of log(sum_{j in g} mu_j / (1 + alpha mu_j))"""
    x, _ = _as_grid(x)
    w = mu[:, :, None] / (1.0 + np.exp(x)[None] * mu[:, :, None])
    return sum(np.log(w[codes == g].sum(axis=0)) for g in range(k))


def objective(c, mu, codes, k, x, log_prior_mean=None, prior_var=None):
    """L(x): the Cox-Reid adjusted profile likelihood, with the prior term if a prior is given; the shape of x"""
    xg, squeeze = _as_grid(x)
    L = sum(t.sum(axis=0) for t in likelihood_terms(c, mu, xg)) - 0.5 * cox_reid(mu, codes, k, xg)
    if log_prior_mean is not None:
        L = L - (xg - np.asarray(log_prior_mean)[:, None]) ** 2 / (2.0 * prior_var)
    return L[:, 0] if squeeze else L


def bound(c, mu, k, x):
    """B of the parity rule: 64 ulp of the magnitudes actually added, plus one per term where lgamma crosses zero"""
    m = c.shape[0]
    mag = sum(np.abs(t).sum(axis=0) for t in likelihood_terms(c, mu, x))[:, 0]
    return 64 * 2.0 ** -53 * (mag + 4 * m + k)


def grid_search(f, lo, hi):
    """the maximiser BY DEFINITION: six rounds of the 64-point grid x_i = lo + (hi - lo) i / 63 on f (G, P) -> (G, P); the first
    largest value at b; the next bracket [x_max(b-1,0), x_min(b+1,63)].  Returns (x, f(x)) of the last round."""
    i = np.arange(GRID, dtype=np.float64)
    rows = np.arange(lo.shape[0])
    for _ in range(ROUNDS):
        x = lo[:, None] + (hi - lo)[:, None] * i / 63.0
        L = f(x)
        b = np.argmax(L, axis=1)
        lo, hi = x[rows, np.maximum(b - 1, 0)], x[rows, np.minimum(b + 1, GRID - 1)]
    return x[rows, b], L[rows, b]


def dispersions(counts, codes, k, s, log_prior_mean=None, prior_var=None, chunk=256):
    """(x, L(x), mu) per gene; NaN for a gene of zeros"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    m, G = c.shape
    mu = fitted_mu(c, codes, k, s)
    x, L = np.full(G, np.nan), np.full(G, np.nan)
    live = np.flatnonzero((c > 0).any(axis=0))
    for a in range(0, live.size, chunk):
        j = live[a:a + chunk]
        prior = None if log_prior_mean is None else np.asarray(log_prior_mean)[j]
        x[j], L[j] = grid_search(lambda xs: objective(c[:, j], mu[:, j], codes, k, xs, prior, prior_var),
                                 np.full(j.size, np.log(MIN_DISP)), np.full(j.size, np.log(max_disp(m))))
    return x, L, mu


def resolved(c, mu, codes, k, x, delta=1e-4, log_prior_mean=None, prior_var=None):
    """the genes whose maximiser is pinned: interior, and L drops by more than 2 B at x -+ delta"""
    m = c.shape[0]
    ok = np.isfinite(x)
    out = np.zeros(x.size, dtype=bool)
    j = np.flatnonzero(ok)
    cj, muj, xj = c[:, j], mu[:, j], x[j]
    prior = None if log_prior_mean is None else np.asarray(log_prior_mean)[j]
    L = objective(cj, muj, codes, k, np.stack([xj - delta, xj, xj + delta], axis=1), prior, prior_var)
    B = bound(cj, muj, k, xj)
    interior = (xj - delta > np.log(MIN_DISP)) & (xj + delta < np.log(max_disp(m)))
    out[j] = interior & (L[:, 1] - L[:, 0] > 2 * B) & (L[:, 1] - L[:, 2] > 2 * B)
    return out


def score(c, s, alpha, q):
    """sum_j (c_j - s_j q) / (1 + alpha s_j q) of one group: c (n, G), s (n,), alpha and q (G,)"""
    sq = s[:, None] * q[None]
    return ((c - sq) / (1.0 + alpha[None] * sq)).sum(axis=0)


def group_fits(counts, codes, k, s, alpha):
    """(q, w, flags), each (G, k): the root of the score in log q by 200 bisection steps on [sum c / (sum s (1 + alpha smax qmax))
    or qmin, qmax] -- far past the last bit --, floored at minmu / max s; a NaN alpha gives NaN"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    G = c.shape[1]
    alpha = np.asarray(alpha, dtype=np.float64)
    q, w, flags = np.full((G, k), np.nan), np.full((G, k), np.nan), np.zeros((G, k), dtype=np.int32)
    live = ~np.isnan(alpha)
    a = np.where(live, alpha, 1.0)
    for g in range(k):
        cg, sg = c[codes == g], s[codes == g]
        qj = cg / sg[:, None]
        qmin, qmax = qj.min(axis=0), qj.max(axis=0)
        root = qmax.copy()
        solve = qmax > qmin
        if solve.any():
            cs, al = cg[:, solve], a[solve]
            lower = cs.sum(axis=0) / (sg.sum() * (1.0 + al * sg.max() * qmax[solve]))
            lo, hi = np.log(np.maximum(qmin[solve], lower)), np.log(qmax[solve])
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                up = score(cs, sg, al, np.exp(mid)) > 0
                lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
            root[solve] = np.exp(0.5 * (lo + hi))
        floor = MIN_MU / sg.max()
        floored = root < floor
        root = np.where(floored, floor, root)
        mu = np.maximum(sg[:, None] * root[None], MIN_MU)
        q[:, g], w[:, g] = root, (mu / (1.0 + a[None] * mu)).sum(axis=0)
        flags[:, g] = np.where(floored, FLOORED, 0)
    q[~live], w[~live], flags[~live] = np.nan, np.nan, 0
    return q, w, flags


def used_for_fit(disp):
    with np.errstate(invalid="ignore"):
        return np.isfinite(disp) & (disp >= 100 * MIN_DISP)


def prior_var(log_disp, log_trend, m, k):
    """(priorVar, varLogDisp) of step 5"""
    use = used_for_fit(np.exp(log_disp)) & np.isfinite(log_trend)
    rho = log_disp[use] - log_trend[use]
    var_log_disp = float((1.4826 * np.median(np.abs(rho - np.median(rho)))) ** 2)
    return max(var_log_disp - float(special.polygamma(1, (m - k) / 2.0)), 0.25), var_log_disp


def outliers(log_disp, log_trend, var_log_disp):
    with np.errstate(invalid="ignore"):
        return log_disp > log_trend + 2.0 * np.sqrt(var_log_disp)


def wald(q, w, first=0, second=1):
    """(log2 fold change second over first, its standard error, the statistic, the two-sided p-value)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        lfc = np.log2(q[:, second]) - np.log2(q[:, first])
        se = np.log2(np.e) * np.sqrt(1.0 / w[:, first] + 1.0 / w[:, second])
        stat = lfc / se
    return lfc, se, stat, 2.0 * stats.norm.sf(np.abs(stat))


# ---- the gene classes of the tests ------------------------------------------------------------------------------------------------
def size_factors(rng, m):
    s = np.exp(rng.normal(0.0, 0.3, m))
    return s / np.exp(np.log(s).mean())


def nb_counts(rng, mean, alpha):
    """negative-binomial draws of the given means (any shape) and dispersion (broadcast): a gamma-mixed Poisson"""
    alpha = np.broadcast_to(alpha, mean.shape)
    return rng.poisson(rng.gamma(1.0 / alpha, alpha * mean)).astype(np.float64)


def nb_class(rng, s, codes, k, G):
    """the issue's generator: base mean log-uniform on [2, 3000], alpha = 0.05 + 2 / base, 20 % of the (gene, group) entries carry
    a fold change exp(N(0, 1))"""
    base = np.exp(rng.uniform(np.log(2.0), np.log(3000.0), G))
    fold = np.where(rng.random((k, G)) < 0.2, np.exp(rng.normal(0.0, 1.0, (k, G))), 1.0)
    mean = s[:, None] * (base[None] * fold)[codes]
    return nb_counts(rng, mean, (0.05 + 2.0 / base)[None])
