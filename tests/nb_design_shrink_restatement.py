"""The apeglm-style shrunken coefficient of the negative-binomial GLM for a general design (K27) restated in numpy / scipy,
vectorised over genes x grid points, by another route than the kernel's: the profile over the p - 1 unshrunk coefficients comes from
a dense Newton iteration through numpy.linalg.solve whose step is halved on the VALUE of the objective (the kernel reads the change
term by term from a Cholesky solve in registers).  Shared by test_nb_design_shrink_args.py, which pins these functions to scipy on
their own, and test_gpu_nb_design_shrink.py, which holds the device to them.  Nothing here imports the product.

Layout: c is samples x genes (rint of the counts), X the m x p design (first column ones), k the shrunk column, s the size factors,
alpha one dispersion per gene; b is the shrunk coefficient, one value per gene (G,) or a row of values per gene (G, T); beta is
(G, p) or (G, T, p) in X's column order, natural-log scale."""
import numpy as np

import nb_design_restatement as DR
import nb_shrink_restatement as SR

GRID, ROUNDS, SIGMA0 = SR.GRID, SR.ROUNDS, SR.SIGMA0
NOT_CONVERGED, AT_BOUND = SR.NOT_CONVERGED, SR.AT_BOUND
TOL, MAX_STEPS, MAX_HALVINGS = 1e-10, 200, 60
beta_k_of, t_of = SR.beta1_of, SR.t_of


def _others(p, k):
    return np.array([l for l in range(p) if l != k])


def _eta(X, s, beta):
    """(m, G, T) for beta (G, T, p)"""
    return np.einsum("jl,gtl->jgt", X, beta) + np.log(s)[:, None, None]


def likelihood_terms(c, X, s, alpha, beta):
    """the two terms of the bracket of P, each (m, G, T), for beta (G, T, p): c log(a mu) and -(c + 1/a) log1p(a mu)"""
    a = np.asarray(alpha, dtype=np.float64)[None, :, None]
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        am = a * np.exp(_eta(X, s, beta))
        cc = c[:, :, None]
        first = np.where(cc > 0, cc * np.log(am), 0.0)
        return first, -(cc + 1.0 / a) * np.log1p(am)


def P(c, X, s, alpha, beta, S, k, sigma0=SIGMA0):
    """the log posterior up to constants at beta (G, p) or (G, T, p); (G,) or (G, T)"""
    beta = np.asarray(beta, dtype=np.float64)
    squeeze = beta.ndim == 2
    bt = beta[:, None, :] if squeeze else beta
    o = _others(X.shape[1], k)
    # (the samples are added in extended precision where numpy has it, as nb_shrink_restatement.P does)
    like = sum(t.sum(axis=0, dtype=np.longdouble) for t in likelihood_terms(c, X, s, alpha, bt))
    out = (like - (bt[:, :, o] ** 2).sum(axis=2) / (2.0 * sigma0 ** 2) - np.log1p((bt[:, :, k] / S) ** 2)).astype(np.float64)
    return out[:, 0] if squeeze else out


def _gram(w, Z):
    """(N, q, q): Z^T diag(w_n) Z for the weights w (m, N)"""
    q = Z.shape[1]
    return (w.T @ (Z[:, :, None] * Z[:, None, :]).reshape(Z.shape[0], q * q)).reshape(-1, q, q)


def profile_step(c, X, s, alpha, beta, k, sigma0=SIGMA0):
    """the Newton step of the inner problem (the p - 1 unshrunk coefficients, beta_k held) at beta, for N problems: c (m, N),
    alpha (N,), beta (N, p) -> (N, p - 1).  Information Z^T W Z + I / sigma0^2 over the other columns Z, w = mu (1 + a c) /
    (1 + a mu)^2; score Z^T (c - mu) / (1 + a mu) - beta_other / sigma0^2."""
    o = _others(X.shape[1], k)
    Z, lam = X[:, o], 1.0 / sigma0 ** 2
    with np.errstate(over="ignore", invalid="ignore"):
        mu = np.exp(X @ beta.T + np.log(s)[:, None])
        inv = 1.0 / (1.0 + alpha[None] * mu)
        r = (c - mu) * inv
        w = (mu * inv) * ((1.0 + alpha[None] * c) * inv)
        H = _gram(w, Z) + lam * np.eye(o.size)[None]
        g = (Z.T @ r).T - lam * beta[:, o]
        bad = ~(np.isfinite(H).all(axis=(1, 2)) & np.isfinite(g).all(axis=1))
        H[bad], g[bad] = np.eye(o.size), np.nan
        return np.linalg.solve(H, g[:, :, None])[:, :, 0]


def _inner_value(c, X, s, alpha, beta, o, lam):
    """what the inner problem maximises, (N,): sum_j [c eta - (c + 1/a) log1p(a e^eta)] - lam / 2 |beta_other|^2"""
    with np.errstate(over="ignore", invalid="ignore"):
        eta = X @ beta.T + np.log(s)[:, None]
        return (c * eta - (c + 1.0 / alpha[None]) * np.log1p(alpha[None] * np.exp(eta))).sum(axis=0) - 0.5 * lam * (beta[:, o] ** 2).sum(axis=1)


def solve_others(c, X, s, alpha, b, k, sigma0=SIGMA0, start=None):
    """the maximiser over the other coefficients at beta_k = b, for N problems: c (m, N), alpha (N,), b (N,) -> (beta (N, p),
    converged (N,)).  start: (N, p) (its column k is not read); default K26's cold start.  Strictly concave, so any path ends at the
    same point: Newton steps, each halved until the value does not fall, to max |step| <= 1e-10."""
    N, p = b.size, X.shape[1]
    o = _others(p, k)
    lam = 1.0 / sigma0 ** 2
    beta = DR.cold_start(c, s, p) if start is None else np.array(start, dtype=np.float64)
    beta[:, k] = b
    conv = np.zeros(N, dtype=bool)
    act = np.arange(N)
    for _ in range(MAX_STEPS):
        if act.size == 0:
            break
        bt, a, cc = beta[act], alpha[act], c[:, act]
        d = profile_step(cc, X, s, a, bt, k, sigma0)
        moved = np.abs(d).max(axis=1)
        v0 = _inner_value(cc, X, s, a, bt, o, lam)
        t, need = np.ones(act.size), ~(moved <= 1e-7)          # (a short step is taken whole: the value cannot tell there)
        for _ in range(MAX_HALVINGS):
            n = np.flatnonzero(need)
            if n.size == 0:
                break
            trial = bt[n]
            trial[:, o] += t[n, None] * d[n]
            v1 = _inner_value(cc[:, n], X, s, a[n], trial, o, lam)
            # (a fall within the rounding of the value itself is no fall: the direction is an ascent direction of a concave function)
            need[n] = ~(np.isfinite(v1) & (v1 >= v0[n] - 1e-13 * (np.abs(v0[n]) + 1.0)))
            t = np.where(need, 0.5 * t, t)
        bt[:, o] += t[:, None] * d
        beta[act] = bt
        with np.errstate(invalid="ignore"):
            done = t * moved <= TOL
        conv[act[done]] = True
        act = act[~done]
    return beta, conv


def profile(c, X, s, alpha, b, S, k, sigma0=SIGMA0, start=None):
    """(p(b), the coefficients there (.., p), whether every inner fit converged); p has the shape of b, (G,) or (G, T).  start: (G, p)"""
    b = np.asarray(b, dtype=np.float64)
    squeeze = b.ndim == 1
    bg = b[:, None] if squeeze else b
    G, T = bg.shape
    first = None if start is None else np.repeat(np.asarray(start, dtype=np.float64), T, axis=0)
    beta, conv = solve_others(np.repeat(c, T, axis=1), X, s, np.repeat(alpha, T), bg.ravel(), k, sigma0, first)
    beta = beta.reshape(G, T, -1)
    val = P(c, X, s, alpha, beta, S, k, sigma0)
    return (val[:, 0], beta[:, 0], bool(conv.all())) if squeeze else (val, beta, bool(conv.all()))


def information(c, X, s, alpha, beta):
    """(G, p, p): X^T W X with w = mu (1 + a c) / (1 + a mu)^2 at beta (G, p), every column"""
    mu = s[:, None] * np.exp(X @ beta.T)
    w = mu * (1.0 + alpha[None] * c) / (1.0 + alpha[None] * mu) ** 2
    return _gram(w, X)


def far_end(beta_k):
    """sg E from K26's coefficient: E = |beta_k| + 1, sg its sign (+ for 0); 1 for a gene left out"""
    beta_k = np.asarray(beta_k, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(beta_k), 1.0, np.where(beta_k >= 0, np.abs(beta_k) + 1.0, -np.abs(beta_k) - 1.0))


def live_genes(c, alpha):
    return ~np.isnan(alpha) & (c > 0).any(axis=0)


def search(counts, X, s, alpha, far, S, k, sigma0=SIGMA0, start=None, chunk=64):
    """the maximiser BY DEFINITION: six rounds of the 64-point grid t_i = lo + (hi - lo) i / 63 from [0, asinh(E / S)] on
    t -> p(sg S sinh t); the first largest value at w; the next bracket [t_max(w-1,0), t_min(w+1,63)].  Returns a dict: beta (G, p),
    p, t (G,), info (G, p, p), flags.  A NaN alpha or a gene of zeros gives NaN and no flags.  start: (G, p), where round 0's inner
    fits begin (a later round's begin at the round before's winner: the optimum does not depend on the start, the time does)."""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    G, p = c.shape[1], X.shape[1]
    alpha, far = np.asarray(alpha, dtype=np.float64), np.asarray(far, dtype=np.float64)
    out = {"beta": np.full((G, p), np.nan), "p": np.full(G, np.nan), "t": np.full(G, np.nan), "info": np.full((G, p, p), np.nan),
           "flags": np.zeros(G, dtype=np.int32)}
    live = np.flatnonzero(live_genes(c, alpha))
    i = np.arange(GRID, dtype=np.float64)
    for at in range(0, live.size, chunk):
        j = live[at:at + chunk]
        cj, aj, fj = c[:, j], alpha[j], far[j]
        rows = np.arange(j.size)
        lo, hi = np.zeros(j.size), np.arcsinh(np.abs(fj) / S)
        at_end = np.ones(j.size, dtype=bool)
        first = None if start is None else np.asarray(start)[j]
        for r in range(ROUNDS):
            t = lo[:, None] + (hi - lo)[:, None] * i / 63.0
            val, beta, conv = profile(cj, X, s, aj, beta_k_of(fj, S, t), S, k, sigma0, first)
            if not conv:
                out["flags"][j] |= NOT_CONVERGED
            w = np.argmax(val, axis=1)
            out["flags"][j] |= np.where(at_end & (w == GRID - 1), AT_BOUND, 0).astype(np.int32)
            at_end &= w == GRID - 1
            first = beta[rows, w]
            lo, hi = t[rows, np.maximum(w - 1, 0)], t[rows, np.minimum(w + 1, GRID - 1)]
        out["beta"][j], out["p"][j], out["t"][j] = beta[rows, w], val[rows, w], t[rows, w]
        out["info"][j] = information(cj, X, s, aj, out["beta"][j])
    return out


def bound(c, X, s, alpha, beta, S, k, sigma0=SIGMA0):
    """B of the parity rule at beta (G, p): 64 ulp of the magnitudes actually added"""
    m = c.shape[0]
    o = _others(X.shape[1], k)
    mag = sum(np.abs(t).sum(axis=0) for t in likelihood_terms(c, X, s, alpha, beta[:, None, :]))[:, 0]
    return 64 * 2.0 ** -53 * (mag + (beta[:, o] ** 2).sum(axis=1) / (2.0 * sigma0 ** 2) + np.log1p((beta[:, k] / S) ** 2) + 4 * m + 2)


def resolved(c, X, s, alpha, far, S, k, found, delta=1e-4, sigma0=SIGMA0):
    """the genes whose maximiser is pinned: the winner is not lane 0 or 63 of the first bracket (t -+ delta lie inside
    [0, asinh(E / S)]), and p drops by more than 2 B at t -+ delta.  found: the dict of search()."""
    out = np.zeros(alpha.size, dtype=bool)
    j = np.flatnonzero(live_genes(c, alpha))
    if j.size == 0:
        return out
    cj, aj, fj = c[:, j], alpha[j], far[j]
    t = found["t"][j]
    ts = np.stack([t - delta, t, t + delta], axis=1)
    val, _, _ = profile(cj, X, s, aj, beta_k_of(fj, S, ts), S, k, sigma0, found["beta"][j])
    B = bound(cj, X, s, aj, found["beta"][j], S, k, sigma0)
    inner = (t - delta > 0.0) & (t + delta < np.arcsinh(np.abs(fj) / S))
    out[j] = inner & (val[:, 1] - val[:, 0] > 2 * B) & (val[:, 1] - val[:, 2] > 2 * B)
    return out


def posterior_sd(beta, info, S, k, sigma0=SIGMA0):
    """the Laplace approximation of the posterior standard deviation of beta_k: sqrt((H^-1)_kk), H = info + the priors' curvature;
    NaN where H is not positive definite"""
    G, p = beta.shape
    sd = np.full(G, np.nan)
    for g in range(G):
        if not (np.isfinite(info[g]).all() and np.isfinite(beta[g]).all()):
            continue
        prior = np.full(p, 1.0 / sigma0 ** 2)
        b = beta[g, k]
        prior[k] = 2.0 * (S * S - b * b) / (S * S + b * b) ** 2
        H = info[g] + np.diag(prior)
        if (np.linalg.eigvalsh(H) > 0).all():
            sd[g] = np.sqrt(np.linalg.inv(H)[k, k])
    return sd


# ---- the gene classes of the tests ------------------------------------------------------------------------------------------------
CLASSES = ["nb", "min disp", "alpha 10", "huge", "group zero", "single", "all zero"]
CASES = [(4, 2, 1, 1.0), (9, 8, 63, 0.3), (12, 4, 65, 0.02), (12, 4, 63, 1.0), (65, 3, 63, 0.3), (130, 5, 65, 1.0)]


def class_counts(rng, s, X, kinds, G):
    """G genes of the classes above, class j % 7 for gene j: (c, alpha, kind).  The dispersions are inputs of the shrinkage."""
    m = s.size
    base = np.exp(rng.uniform(np.log(2.0), np.log(3000.0), G))
    c = DR.nb_class(rng, s, X, kinds, G)
    alpha = np.clip(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1.0), DR.MIN_DISP, DR.max_disp(m))
    kind = np.arange(G) % len(CLASSES)
    mean = s[:, None] * base[None]
    for j in range(G):
        what = CLASSES[kind[j]]
        if what == "min disp":
            alpha[j] = DR.MIN_DISP
        elif what == "alpha 10":
            c[:, j] = DR.nb_counts(rng, mean[:, j], 10.0)
            alpha[j] = 10.0
        elif what == "huge":
            c[:, j] = DR.nb_counts(rng, 2e6 * s, 0.01)
            alpha[j] = 0.01
        elif what == "group zero":
            c[X[:, -1] == 1, j] = 0.0
        elif what == "single":
            c[:, j] = 0.0
            c[rng.integers(m), j] = 1.0 + rng.integers(40)
        elif what == "all zero":
            c[:, j] = 0.0
            alpha[j] = np.nan
    if not (c[:, kind == 0] > 0).any(axis=0).all():
        raise RuntimeError("an NB-class gene is all zero")
    return c, alpha, kind


def case_inputs(m, p, G, S):
    """the inputs of a case of test_gpu_nb_design_shrink.py, the group column last: a dict of s, X, kinds, c, alpha, kind"""
    rng = np.random.default_rng(27000 + 100 * m + 10 * p + G)
    s = DR.size_factors(rng, m)
    X, kinds = DR.make_design(rng, m, p)
    c, alpha, kind = class_counts(rng, s, X, kinds, G)
    return dict(m=m, p=p, G=G, S=S, s=s, X=X, kinds=kinds, c=c, alpha=alpha, kind=kind)
