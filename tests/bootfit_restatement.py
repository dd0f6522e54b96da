"""numpy restatement of the bootstrap Huber fits (K10, engine.bootstrap_huber_fits) and of gene_cluster_differentiation's host
stages, written from the behaviour they describe.

A bootstrap fit regresses y (in its own order) on resampled times x[idx]; it is the optimum of scikit-learn's HuberRegressor
objective (tests/trajfit_restatement.huber_objective).  Unlike trajfit_restatement.huber this solver does not need three distinct
times: it works in u = (x - m) / s of the BASE times (all resamples share the map), starts from the penalised least-squares fit
and keeps the penalty alpha ||w||^2 in every Newton step, so a resample with one or two distinct times still has its unique
optimum.  The stop rule is the restatement's (sum |projected gradient|) * sigma <= tol * objective, or no lower objective along a
descent direction; the last Newton steps are polished with scipy's L-BFGS-B as a cross-check (``huber_opt`` returns the lower)."""
import numpy as np
from scipy import optimize

from trajfit_restatement import ALPHA, MODELS, SIGMA_MIN, design, huber_objective


def _basis(u, model, kappa, qs):
    if model == "linear":
        return np.column_stack([np.ones_like(u), u])
    if model == "linear_quadratic":
        return np.column_stack([np.ones_like(u), u, u * u])
    return np.column_stack([np.ones_like(u), (u * u + kappa * u) * qs])


def _to_params(model, m, s, kappa, qs):
    """T: params on [1, f(x)] = T gamma"""
    if model == "linear":
        return np.array([[1.0, -m / s], [0.0, 1.0 / s]])
    if model == "linear_quadratic":
        return np.array([[1.0, -m / s, m * m / (s * s)], [0.0, 1.0 / s, -2.0 * m / (s * s)], [0.0, 0.0, 1.0 / (s * s)]])
    # (u^2 + kappa u) qs with u = (x - m) / s, kappa = 2 m / s: (x^2 - m^2) qs / s^2
    return np.array([[1.0, -m * m * qs / (s * s)], [0.0, qs / (s * s)]])


def huber_opt(x_base, xr, y, model, epsilon=1.35, tol=1e-12, max_iter=200):
    """The penalised Huber optimum of y on the times xr (a resample of x_base).  Returns (params, sigma, objective)."""
    x_base = np.asarray(x_base, dtype=np.float64)
    xr = np.asarray(xr, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    m = x_base.mean()
    s = np.abs(x_base - m).max()
    s = s if s > 0 else 1.0
    kappa = 2 * m / s
    qs = 1.0 / (1.0 + abs(kappa))
    B = _basis((xr - m) / s, model, kappa, qs)
    T = _to_params(model, m, s, kappa, qs)
    Pen = ALPHA * T[1:].T @ T[1:]
    n, p = B.shape
    if np.all(y == y[0]):
        prm = np.zeros(p)
        prm[0] = y[0]
        return prm, SIGMA_MIN, huber_objective(xr, y, model, prm, SIGMA_MIN, epsilon)
    gam = np.linalg.solve(B.T @ B + Pen, B.T @ y)
    res = y - B @ gam
    sse = res @ res
    sig = max(np.sqrt(sse / n) if sse > 1e-8 * (y @ y) else np.sqrt((y @ y) / n), SIGMA_MIN)

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
            break
        t, F, g, H = best
        gam, sig = gam + t * d[:p], max(sig + t * d[p], SIGMA_MIN)
    # cross-check: L-BFGS-B from the Newton point on (gamma, log-free sigma with its bound)
    lb = optimize.minimize(lambda z: evaluate(z[:p], z[p])[0], np.r_[gam, sig], jac=lambda z: evaluate(z[:p], z[p])[1],
                           method="L-BFGS-B", bounds=[(None, None)] * p + [(SIGMA_MIN, None)],
                           options=dict(gtol=1e-14, ftol=1e-16, maxiter=200))
    if lb.fun < F:
        gam, sig = lb.x[:p], lb.x[p]
    prm = T @ gam
    return prm, sig, huber_objective(xr, y, model, prm, sig, epsilon)


def objective(xr, y, model, params, sigma, epsilon=1.35):
    p = 3 if model == "linear_quadratic" else 2
    return huber_objective(xr, y, model, np.asarray(params, dtype=np.float64)[:p], sigma, epsilon)


__all__ = ["huber_opt", "objective", "design", "MODELS", "SIGMA_MIN"]
