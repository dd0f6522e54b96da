"""numpy / scipy restatement of pilotpy's trajectory model fits (fit_best_model / fit_model_activity,
pilotpy/tools/Cell_gene_selection.py; cell_importance / genes_importance, Trajectory.py), written from the behaviour they
describe: three models with an intercept (linear [x], linear_quadratic [x, x^2], quadratic [x^2]) fitted by OLS or to the
OPTIMUM of scikit-learn's HuberRegressor objective, adjusted and modified R^2, t-test p-values, the model choice, slope, pattern
and the Pearson test.  Held to scikit-learn / scipy (L-BFGS-B for the Huber optimum) by tests/test_trajectory_fit_args.py.  Least
squares and the Huber solve work in numpy.polynomial's scaled domain (well conditioned whatever the range of x)."""
import numpy as np
from numpy.polynomial import Polynomial
from scipy import stats

MODELS = ("linear", "linear_quadratic", "quadratic")
ALPHA = 1e-4
SIGMA_MIN = 10 * np.finfo(np.float64).eps


def design(x, model):
    """Z = [1, f(x)]"""
    x = np.asarray(x, dtype=np.float64)
    f = {"linear": [x], "linear_quadratic": [x, x * x], "quadratic": [x * x]}[model]
    return np.column_stack([np.ones_like(x)] + f)


def _domain(x, model):
    """(v, deg): the polynomial variable and degree of the model: y = poly(v)"""
    x = np.asarray(x, dtype=np.float64)
    return (x * x, 1) if model == "quadratic" else (x, 1 if model == "linear" else 2)


def _to_params(poly, deg):
    c = poly.convert().coef
    return np.r_[c, np.zeros(deg + 1 - c.size)]


def ols(x, y, model):
    """(params on [1, f(x)], predictions)"""
    v, deg = _domain(x, model)
    P = Polynomial.fit(v, y, deg)
    return _to_params(P, deg), P(v)


def huber_objective(x, y, model, params, sigma, epsilon):
    """scikit-learn's HuberRegressor objective at (params = [c, w], sigma)"""
    r = np.asarray(y, dtype=np.float64) - design(x, model) @ params
    out = np.abs(r) > epsilon * sigma
    w = params[1:]
    return (len(r) * sigma + np.sum(r[~out] ** 2) / sigma + np.sum(2 * epsilon * np.abs(r[out]) - epsilon ** 2 * sigma)
            + ALPHA * w @ w)


def _huber_setup(x, model):
    """the model in numpy.polynomial's mapped variable t = off + scl v: basis B (n x p), params = T gamma, penalty on gamma"""
    v, deg = _domain(x, model)
    off, scl = Polynomial.fit(v, np.zeros_like(v), deg).mapparms()
    t = off + scl * v
    B = np.column_stack([t ** k for k in range(deg + 1)])
    T = np.zeros((deg + 1, deg + 1))                   # column k: the coefficients of t^k = (off + scl v)^k in powers of v
    for k in range(deg + 1):
        c = Polynomial([off, scl]) ** k
        T[:c.coef.size, k] = c.coef
    return B, T, ALPHA * T[1:].T @ T[1:]


def huber(x, y, model, epsilon=1.35, tol=1e-12, max_iter=200):
    """The optimum of the Huber objective: Newton directions on (gamma, sigma) with a bracketing line search on the directional
    derivative, sigma projected onto its bound.  Stops when (sum |projected gradient|) * sigma <= tol * objective, or when no
    lower objective exists in floating point along the direction.  Returns (params, sigma, objective, converged)."""
    y = np.asarray(y, dtype=np.float64)
    B, T, Pen = _huber_setup(x, model)
    n, p = B.shape
    if np.all(y == y[0]):
        g = np.zeros(p)
        g[0] = y[0]
        return T @ g, SIGMA_MIN, huber_objective(x, y, model, T @ g, SIGMA_MIN, epsilon), True
    gam = np.linalg.lstsq(B, y, rcond=None)[0]
    sig = max(np.sqrt(np.mean((y - B @ gam) ** 2)), SIGMA_MIN)

    def evaluate(gam, sig):
        r = y - B @ gam
        inl = np.abs(r) <= epsilon * sig
        ri, Bi, sg = r[inl], B[inl], np.sign(r[~inl])
        F = (n * sig + ri @ ri / sig + 2 * epsilon * np.abs(r[~inl]).sum() - epsilon ** 2 * sig * (~inl).sum()
             + gam @ Pen @ gam)
        g = np.r_[-2 * Bi.T @ ri / sig - 2 * epsilon * B[~inl].T @ sg + 2 * Pen @ gam,
                  n - ri @ ri / sig ** 2 - epsilon ** 2 * (~inl).sum()]
        H = np.zeros((p + 1, p + 1))
        H[:p, :p] = 2 * Bi.T @ Bi / sig + 2 * Pen
        H[:p, p] = H[p, :p] = 2 * Bi.T @ ri / sig ** 2
        H[p, p] = 2 * ri @ ri / sig ** 3
        return F, g, H

    F, g, H = evaluate(gam, sig)
    done = False
    for _ in range(max_iter + 1):
        bound = sig <= SIGMA_MIN and g[p] > 0
        gp = g.copy()
        Hr = H + 1e-10 * np.abs(np.diag(H)).max() * np.eye(p + 1)
        if bound:
            gp[p] = 0.0
            Hr[p, :] = 0.0
            Hr[:, p] = 0.0
            Hr[p, p] = 1.0
        if np.abs(gp).sum() * sig <= tol * abs(F):
            done = True
            break
        d = np.linalg.solve(Hr, -gp)
        if gp @ d >= 0:
            d = -gp
        s0 = gp @ d
        tmax = np.inf if d[p] >= 0 else (sig - SIGMA_MIN) / -d[p]
        lo, flo, hi, fhi, t, best = 0.0, s0, None, None, min(1.0, tmax), None
        for _ in range(60):
            Ft, gt, Ht = evaluate(gam + t * d[:p], max(sig + t * d[p], SIGMA_MIN))
            st = gt @ d
            if Ft <= F and abs(st) <= 0.1 * abs(s0):
                best = (t, Ft, gt, Ht)
                break
            if st < 0:
                if Ft <= F:
                    best = (t, Ft, gt, Ht)
                lo, flo = t, st
                if hi is None:
                    if t >= tmax:
                        break
                    t = min(4 * t, tmax)
                    continue
            else:
                hi, fhi = t, st
            t = lo + (hi - lo) * min(max(-flo / (fhi - flo), 0.05), 0.95)
        if best is None:
            done = True                               # no lower objective in floating point along a descent direction
            break
        t, F, g, H = best
        gam, sig = gam + t * d[:p], max(sig + t * d[p], SIGMA_MIN)
    params = T @ gam
    return params, sig, huber_objective(x, y, model, params, sig, epsilon), done


def xtx_inv_diag(x, model):
    """diag((Z^T Z)^-1) through a QR of the column-scaled Z"""
    Z = design(x, model)
    s = np.abs(Z).max(axis=0)
    R = np.linalg.qr(Z / s, mode="r")
    Ri = np.linalg.inv(R)
    return (Ri ** 2).sum(axis=1) / s ** 2


def fit_one(x, y, model, kind="ols", epsilon=1.35):
    """fit_model_activity: dict(params, pvalues, rsquared_adj, mod_rsquared_adj, sigma)"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    sigma = None
    if kind == "ols":
        params, pred = ols(x, y, model)
    else:
        params, sigma, _, _ = huber(x, y, model, epsilon)
        pred = design(x, model) @ params
    q = params.size - 1
    p = q + 1
    e = y - pred
    sse = e @ e
    const = np.all(y == y[0])
    sst = 0.0 if const else np.sum((y - y.mean()) ** 2)
    if sst > 0:
        r2 = 1 - sse / sst
    else:
        r2 = 1.0 if sse == 0 else 0.0
    ae = np.abs(e)
    msse = np.sum(np.where(ae < 1.35, 0.5 * e * e, 1.35 * (ae - 0.675)))
    with np.errstate(divide="ignore", invalid="ignore"):
        mr2 = 1 - np.float64(msse) / np.float64(sst)
        mse = sse / (n - p)
        t = params / np.sqrt(mse * xtx_inv_diag(x, model))
    pv = 2 * (1 - stats.t.cdf(np.abs(t), n - p))
    f = (n - 1) / (n - q - 1)
    return dict(params=params, pvalues=pv, rsquared_adj=1 - (1 - r2) * f, mod_rsquared_adj=1 - (1 - mr2) * f, sigma=sigma)


def pearson(x, y):
    if np.all(y == y[0]):
        return np.nan, np.nan
    r = stats.pearsonr(x, y)
    return float(r[0]), float(r[1])


def best_model(x, y, pval_thr=0.05, modify_r2=False, kind="ols", epsilon=1.35):
    """fit_best_model for one target: (chosen index or -1, per-model fits, slope, pattern string, (r, p)), plus the deciding
    margin: the smallest distance of a p-value to pval_thr, or between the chosen R^2 and a competitor's"""
    fits = [fit_one(x, y, m, kind, epsilon) for m in MODELS]
    best, chosen = -1000.0, -1
    margin = np.inf
    key = "mod_rsquared_adj" if modify_r2 else "rsquared_adj"
    elig = []
    for k, f in enumerate(fits):
        pv = f["pvalues"]
        margin = min(margin, np.nanmin(np.abs(pv - pval_thr)) if np.isfinite(pv).any() else np.inf)
        ok = bool(np.all(pv <= pval_thr))
        elig.append(ok)
        if ok and f[key] > best:
            best, chosen = f[key], k
    for k, f in enumerate(fits):
        if elig[k] and k != chosen and np.isfinite(f[key]):
            margin = min(margin, abs(f[key] - best))
    slope, pattern = np.nan, None
    if chosen >= 0:
        prm = fits[chosen]["params"]
        xl = np.linspace(x.min(), x.max())
        curve = design(xl, MODELS[chosen]) @ prm
        slope = (curve[-1] - curve[0]) / (xl[-1] - xl[0])
        if chosen == 1:
            pattern = "linear %s quadratic %s" % ("up" if prm[1] >= 0 else "down", "up" if prm[2] >= 0 else "down")
        else:
            pattern = "%s %s" % (MODELS[chosen], "up" if prm[1] >= 0 else "down")
    return dict(chosen=chosen, fits=fits, slope=slope, pattern=pattern, pearson=pearson(x, y), margin=margin)


def table(results, names, id_col, p_val, modify_r2=False):
    """save_data's table from per-target best_model results: sorted by the chosen R^2 (Python's stable sort, descending),
    BH-adjusted Pearson p (scipy), rows with adjusted p <= p_val.  Returns (rows as a list of dicts, sorted names)."""
    key = "mod_rsquared_adj" if modify_r2 else "rsquared_adj"
    sel = [(nm, r) for nm, r in zip(names, results) if r["chosen"] >= 0]
    sel = sorted(sel, key=lambda it: it[1]["fits"][it[1]["chosen"]][key], reverse=True)
    if not sel:
        return [], []
    adj = stats.false_discovery_control([r["pearson"][1] for _, r in sel], method="bh")
    rows = []
    for (nm, r), a in zip(sel, adj):
        f = r["fits"][r["chosen"]]
        prm = np.r_[f["params"], np.nan][:3]
        rows.append({id_col: nm, "Expression pattern": r["pattern"], "Slope": r["slope"], "Fitted function": MODELS[r["chosen"]],
                     "Intercept": prm[0], "Treat": prm[1], "Treat2": prm[2], "adjusted P-value": a,
                     "R-squared": f["rsquared_adj"], "mod_rsquared_adj": f["mod_rsquared_adj"]})
    return [row for row in rows if row["adjusted P-value"] <= p_val], [nm for nm, _ in sel]


def normalize_log1p(X, target_sum=1e4):
    """scanpy's normalize_total(target_sum) + log1p as restated here (UNPINNED: scanpy is not installed): f64 row totals"""
    X = np.asarray(X, dtype=np.float64)
    tot = X.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(tot > 0, target_sum / tot, 0.0)
    return np.log1p(X * scale)
