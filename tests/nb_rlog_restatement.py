"""The regularised log transform (K24) restated in numpy / scipy.  Shared by test_nb_rlog_args.py, which pins these
functions to scipy on their own, and test_gpu_nb_rlog.py, which holds the device to them.  Nothing here imports the product.

Per gene, with c the rounded counts of the m samples, s the size factors, alpha the dispersion, lambda = ln2^2 / prior_var and
lambda0 = 1e-6 ln2^2, x = (b0, b_1 .. b_m) and eta_j = b0 + b_j + log s_j:
    P(x) = sum_j [c_j eta_j - (c_j + 1/alpha) log1p(alpha e^{eta_j})] - lambda/2 sum_j b_j^2 - lambda0/2 b0^2
Two routes to its maximiser: the DENSE one (value, gradient, the (m + 1)^2 Hessian, numpy.linalg.solve, halving) one gene at a
time, and the ARROWHEAD one, the device's iteration (the Schur complement of the diagonal block) vectorised over genes, for the
sample counts where a dense Hessian per gene is too much.  Also the weighted-quantile rule of the prior variance and the PCA tail.

Layout: c is samples x genes; x0 / b0 one value per gene, b samples x genes."""
import numpy as np
from scipy import stats

import nb_glm_restatement as RR

LN2 = np.log(2.0)
LAMBDA0 = 1e-6 * LN2 ** 2
TOL, MAX_ITERS, MAX_HALVINGS = 1e-10, 100, 20
NOT_CONVERGED = RR.NOT_CONVERGED


def ridge(prior_var):
    return LN2 ** 2 / prior_var


def blind_dispersions(counts, s, **kw):
    """K22's restatement with the one group of the design `~ 1`: (x, L(x), mu)"""
    return RR.dispersions(counts, np.zeros(s.size, dtype=np.int64), 1, s, **kw)


# ---- the dense route, one gene -----------------------------------------------------------------------------------------------------
def P(c, s, alpha, lam, b0, b):
    eta = b0 + b + np.log(s)
    return float((c * eta - (c + 1.0 / alpha) * np.logaddexp(0.0, np.log(alpha) + eta)).sum() - 0.5 * lam * (b * b).sum()
                 - 0.5 * LAMBDA0 * b0 * b0)


def gradient(c, s, alpha, lam, b0, b):
    """dP / d(b0, b_1 .. b_m)"""
    mu = np.exp(b0 + b + np.log(s))
    r = (c - mu) / (1.0 + alpha * mu)
    return np.append(r.sum() - LAMBDA0 * b0, r - lam * b)


def hessian(c, s, alpha, lam, b0, b):
    """minus the second derivatives of P: positive definite"""
    mu = np.exp(b0 + b + np.log(s))
    w = mu * (1.0 + alpha * c) / (1.0 + alpha * mu) ** 2
    H = np.zeros((c.size + 1, c.size + 1))
    H[0, 0] = w.sum() + LAMBDA0
    H[0, 1:] = H[1:, 0] = w
    H[np.arange(1, c.size + 1), np.arange(1, c.size + 1)] = w + lam
    return H


def dense_step(c, s, alpha, lam, b0, b):
    """the Newton step at (b0, b): (m + 1,)"""
    return np.linalg.solve(hessian(c, s, alpha, lam, b0, b), gradient(c, s, alpha, lam, b0, b))


def dense_fit(c, s, alpha, prior_var, tol=1e-13, max_iters=200):
    """(b0, b, iterations) of one live gene by plain dense Newton steps, halved while P falls (a non-finite P is a fall) unless the
    step is below 1e-6 already, where P no longer resolves it; whoever calls this checks the residual (dense_step) of the result"""
    lam = ridge(prior_var)
    b0, b = float(np.log((c / s).mean())), np.zeros(c.size)
    now = P(c, s, alpha, lam, b0, b)
    for it in range(1, max_iters + 1):
        step = dense_step(c, s, alpha, lam, b0, b)
        t = 1.0
        for _ in range(60):
            with np.errstate(over="ignore", invalid="ignore"):
                new = P(c, s, alpha, lam, b0 + t * step[0], b + t * step[1:])
            if (np.isfinite(new) and new >= now) or np.abs(t * step).max() < 1e-6:
                break
            t *= 0.5
        b0, b, now = b0 + t * step[0], b + t * step[1:], new
        if np.abs(t * step).max() <= tol:
            break
    return b0, b, it


def dense_rlog(counts, s, alpha, prior_var):
    """(rlog (m, G), intercept (G,), the largest dense Newton step left at each live gene's result (G,)): the optimum, log2 scale;
    0 and a NaN intercept for a gene of zeros, NaN for a NaN dispersion"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    m, G = c.shape
    out, intercept, left = np.zeros((m, G)), np.full(G, np.nan), np.zeros(G)
    for j in range(G):
        if np.isnan(alpha[j]):
            out[:, j] = np.nan
        elif (c[:, j] > 0).any():
            b0, b, _ = dense_fit(c[:, j], s, alpha[j], prior_var)
            out[:, j], intercept[j] = (b0 + b) / LN2, b0 / LN2
            left[j] = np.abs(dense_step(c[:, j], s, alpha[j], ridge(prior_var), b0, b)).max()
    return out, intercept, left


def coefficients(rlog, intercept):
    """(b0, b) on the natural-log scale from a result on the log2 scale"""
    b0 = intercept * LN2
    return b0, rlog * LN2 - b0[None]


def dense_step_at(counts, s, alpha, prior_var, rlog, intercept, genes):
    """the largest dense Newton step at a result, for each of `genes`"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    b0, b = coefficients(rlog, intercept)
    return np.array([np.abs(dense_step(c[:, j], s, alpha[j], ridge(prior_var), b0[j], b[:, j])).max() for j in genes])


# ---- the arrowhead route, vectorised over genes ------------------------------------------------------------------------------------
def _terms(c, ls, alpha, lam, b0, b):
    mu = np.exp(b0[None] + b + ls)
    inv = 1.0 / (1.0 + alpha[None] * mu)
    r = (c - mu) * inv
    w = (mu * inv) * ((1.0 + alpha[None] * c) * inv)
    return r, w, r - lam * b, w + lam, alpha[None] * mu * inv


def arrowhead_step(c, s, alpha, prior_var, b0, b):
    """(d0 (G,), d (m, G)): the Newton step through the Schur complement of the diagonal block"""
    lam = ridge(prior_var)
    r, w, g, h, _ = _terms(c, np.log(s)[:, None], alpha, lam, b0, b)
    d0 = (r.sum(axis=0) - LAMBDA0 * b0 - (w * g / h).sum(axis=0)) / (w.sum(axis=0) + LAMBDA0 - (w * w / h).sum(axis=0))
    return d0, (g - w * d0[None]) / h


def _change(c, alpha, lam, b0, b, d0, d, rho, t):
    """P(b0 + t d0, b + t d) - P(b0, b), term by term"""
    D, td, t0 = t[None] * (d0[None] + d), t[None] * d, t * d0
    with np.errstate(over="ignore", invalid="ignore"):
        part = c * D - (c + 1.0 / alpha[None]) * np.log1p(rho * np.expm1(D)) - 0.5 * lam * td * (2.0 * b + td)
        return part.sum(axis=0) - 0.5 * LAMBDA0 * t0 * (2.0 * b0 + t0)


def arrowhead_rlog(counts, s, alpha, prior_var):
    """the device's iteration: dict(rlog (m, G), intercept, steps, flags, halvings)"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    m, G = c.shape
    lam, ls = ridge(prior_var), np.log(s)[:, None]
    dead = np.isnan(alpha)
    live = ~dead & (c > 0).any(axis=0)
    b0, b = np.full(G, np.nan), np.zeros((m, G))
    steps, flags, halvings = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    active = np.flatnonzero(live)
    b0[active] = np.log((c[:, active] / s[:, None]).mean(axis=0))
    for it in range(1, MAX_ITERS + 1):
        if not active.size:
            break
        cj, a, B0, B = c[:, active], alpha[active], b0[active], b[:, active]
        r, w, g, h, rho = _terms(cj, ls, a, lam, B0, B)
        d0 = (r.sum(axis=0) - LAMBDA0 * B0 - (w * g / h).sum(axis=0)) / (w.sum(axis=0) + LAMBDA0 - (w * w / h).sum(axis=0))
        d = (g - w * d0[None]) / h
        t, todo = np.ones(active.size), np.ones(active.size, dtype=bool)
        for halving in range(MAX_HALVINGS + 1):
            change = _change(cj, a, lam, B0, B, d0, d, rho, t)
            todo &= ~(np.isfinite(change) & (change >= 0)) & ~(np.maximum(np.abs(d0), np.abs(d).max(axis=0)) <= TOL)
            if halving == MAX_HALVINGS or not todo.any():
                break
            t[todo] *= 0.5
            halvings[active[todo]] += 1
        b[:, active], b0[active], steps[active] = B + t[None] * d, B0 + t * d0, it
        active = active[~(t * np.maximum(np.abs(d0), np.abs(d).max(axis=0)) <= TOL)]
    flags[active] = NOT_CONVERGED
    out = (b0[None] + b) / LN2
    out[:, ~live & ~dead] = 0.0
    return dict(rlog=out, intercept=b0 / LN2, steps=steps, flags=flags, halvings=halvings)


# ---- the prior variance --------------------------------------------------------------------------------------------------------------
def weighted_upper_quantile(x, weight, upper=0.05):
    """Hmisc's wtd.quantile(x, weight, 1 - upper, normwt = FALSE): the weights of equal x summed, then the type-7 rule on their
    running sum"""
    order = np.argsort(x, kind="stable")
    xs, ws = x[order], weight[order]
    values, first = np.unique(xs, return_index=True)
    cum = np.cumsum(np.add.reduceat(ws, first))
    W = cum[-1]
    o = 1.0 + (W - 1.0) * (1.0 - upper)
    low = max(np.floor(o), 1.0)
    high = min(low + 1.0, W)
    f = o % 1.0

    def q(t):
        at = np.flatnonzero(cum >= t)
        return values[at[0]] if at.size else values[-1]

    return (1.0 - f) * q(low) + f * q(high)


def prior_var(counts, s, base_mean, disp_fit, upper=0.05):
    c = np.rint(np.asarray(counts, dtype=np.float64))
    use = base_mean > 0
    x = np.abs(np.log2(c[:, use] / s[:, None] + 0.5) - np.log2(base_mean[use] + 0.5)[None])
    weight = np.repeat((1.0 / (1.0 / base_mean[use] + disp_fit[use]))[None], c.shape[0], axis=0)
    Q = weighted_upper_quantile(x.ravel(), weight.ravel(), upper)
    return float((Q / stats.norm.ppf(1.0 - upper / 2.0)) ** 2)


# ---- the PCA tail --------------------------------------------------------------------------------------------------------------------
def pca_tail(X, variance_threshold=0.2, n_components=2):
    """(scores, variance ratio, kept columns): the genes with a ddof-0 variance above the threshold, the SVD of the centred table,
    the loading of largest magnitude of every component positive"""
    X = np.asarray(X, dtype=np.float64)
    kept = np.flatnonzero(X.var(axis=0) > variance_threshold)
    Z = X[:, kept] - X[:, kept].mean(axis=0)
    U, sv, Vt = np.linalg.svd(Z, full_matrices=False)
    sign = np.sign(Vt[np.arange(Vt.shape[0]), np.abs(Vt).argmax(axis=1)])
    scores = (U * sv[None]) * sign[None]
    return scores[:, :n_components], (sv ** 2 / (sv ** 2).sum())[:n_components], kept


# ---- the gene classes of the tests ---------------------------------------------------------------------------------------------------
CLASSES = ["nb", "min disp", "alpha 10", "huge", "single", "single 50000", "mean 0.3", "all zero", "nan disp"]


def gene_classes(rng, s, G):
    """G genes of the classes above, class j % 9 for gene j: (counts (m, G), dispersions (G,), class index (G,))"""
    m = s.size
    codes = np.zeros(m, dtype=np.int64)
    base = np.exp(rng.uniform(np.log(2.0), np.log(3000.0), G))
    c = RR.nb_class(rng, s, codes, 1, G)
    alpha = np.clip(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1.0), RR.MIN_DISP, RR.max_disp(m))
    kind = np.arange(G) % len(CLASSES)
    mean = s[:, None] * base[None]
    for j in range(G):
        what = CLASSES[kind[j]]
        if what == "min disp":
            alpha[j] = RR.MIN_DISP
        elif what == "alpha 10":
            c[:, j] = RR.nb_counts(rng, mean[:, j], 10.0)
            if not c[:, j].any():
                c[rng.integers(m), j] = 1.0
            alpha[j] = 10.0
        elif what == "huge":
            c[:, j] = RR.nb_counts(rng, 2e6 * s, 0.01)
            alpha[j] = 0.01
        elif what == "single":
            c[:, j] = 0.0
            c[rng.integers(m), j] = 1.0 + rng.integers(40)
        elif what == "single 50000":
            c[:, j] = 0.0
            c[rng.integers(m), j] = 50000.0
        elif what == "mean 0.3":
            c[:, j] = rng.poisson(0.3 * s)
            if not c[:, j].any():
                c[rng.integers(m), j] = 1.0
            alpha[j] = 0.5
        elif what == "all zero":
            c[:, j] = 0.0
        elif what == "nan disp":
            alpha[j] = np.nan
    return c, alpha, kind
