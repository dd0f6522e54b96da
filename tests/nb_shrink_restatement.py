"""The apeglm-style shrunken fold change of the two-group negative-binomial model (K23) restated in numpy / scipy,
vectorised over genes x grid points.  Shared by test_nb_shrink_args.py, which pins these functions to scipy on their own, and
test_gpu_nb_shrink.py, which holds the device to them.  Nothing here imports the product.

Layout: c is samples x genes (rint of the counts), codes 0 / 1 per sample (1: the numerator group), s the size factors, alpha one
dispersion per gene; b0 and b1 are one value per gene (G,) or a row of values per gene (G, P), on the natural-log scale."""
import numpy as np
from scipy import optimize

import nb_glm_restatement as RR

GRID, ROUNDS, SIGMA0, FAR_FLOORED = 64, 6, 15.0, 30.0
NOT_CONVERGED, FLOORED, AT_BOUND = 1, 2, 4


def _grid(x):
    x = np.asarray(x, dtype=np.float64)
    return (x[:, None], True) if x.ndim == 1 else (x, False)


def _mu(codes, s, b0, b1):
    """(m, G, P): s_j exp(b0 + b1 [j in group 1])"""
    return s[:, None, None] * np.exp(b0[None] + np.where(codes == 1, 1.0, 0.0)[:, None, None] * b1[None])


def likelihood_terms(c, codes, s, alpha, b0, b1):
    """the two terms of the bracket of P, each (m, G, P): c log(a mu) and -(c + 1/a) log1p(a mu)"""
    b0, _ = _grid(b0)
    b1, _ = _grid(b1)
    a = np.asarray(alpha, dtype=np.float64)[None, :, None]
    am = a * _mu(codes, s, b0, b1)
    cc = c[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.where(cc > 0, cc * np.log(am), 0.0)
    return first, -(cc + 1.0 / a) * np.log1p(am)


def P(c, codes, s, alpha, b0, b1, S, sigma0=SIGMA0):
    """the log posterior up to constants; the shape of b0"""
    g0, squeeze = _grid(b0)
    g1, _ = _grid(b1)
    # (the samples are added in extended precision where numpy has it: a float64 reduction over the first axis adds row after row,
    # and at 4096 samples its rounding alone reaches half of the parity bound B)
    like = sum(t.sum(axis=0, dtype=np.longdouble) for t in likelihood_terms(c, codes, s, alpha, g0, g1))
    out = (like - g0 ** 2 / (2.0 * sigma0 ** 2) - np.log1p((g1 / S) ** 2)).astype(np.float64)
    return out[:, 0] if squeeze else out


def score(c, codes, s, alpha, b0, b1, sigma0=SIGMA0):
    """dP / db0, the shape of b0 as a grid"""
    mu = _mu(codes, s, b0, b1)
    return ((c[:, :, None] - mu) / (1.0 + alpha[None, :, None] * mu)).sum(axis=0) - b0 / sigma0 ** 2


def bracket(c, codes, s, b1, sigma0=SIGMA0):
    """(lo, hi) holding the root of the score in b0: above max(0, log max_j c_j / (s_j e^{b1 [g = 1]})) every term is <= 0; below
    -max(1, log(sigma0^2 sum_j s_j e^{b1 [g = 1]})) the likelihood terms sum to more than -sum mu >= b0 / sigma0^2"""
    q = c / s[:, None]
    with np.errstate(divide="ignore"):
        lq0, lq1 = np.log(q[codes == 0].max(axis=0)), np.log(q[codes == 1].max(axis=0))
    top = np.maximum(np.maximum(lq0[:, None], lq1[:, None] - b1), 0.0)
    low = np.log(sigma0 ** 2 * (s[codes == 0].sum() + np.exp(b1) * s[codes == 1].sum()))
    return -np.maximum(low, 1.0) - 1.0, top + 1.0


def solve_b0(c, codes, s, alpha, b1, sigma0=SIGMA0):
    """the root of the score in b0 at b1 by 200 bisection steps on the bracket (ended early once no bound moves, which changes
    nothing: every later step would return the same pair); the shape of b1"""
    g1, squeeze = _grid(b1)
    lo, hi = bracket(c, codes, s, g1, sigma0)
    lo, hi = np.broadcast_to(lo, g1.shape).copy(), np.broadcast_to(hi, g1.shape).copy()
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if ((mid == lo) | (mid == hi)).all():
            break
        up = score(c, codes, s, alpha, mid, g1, sigma0) > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    out = 0.5 * (lo + hi)
    return out[:, 0] if squeeze else out


def profile(c, codes, s, alpha, b1, S, sigma0=SIGMA0):
    """(p(b1), the b0 there), the shape of b1"""
    b0 = solve_b0(c, codes, s, alpha, b1, sigma0)
    return P(c, codes, s, alpha, b0, b1, S, sigma0), b0


def weights(c, codes, s, alpha, b0, b1):
    """(w0, w1): the groups' observed information sum_j mu_j (1 + a c_j) / (1 + a mu_j)^2 at (b0, b1), each (G,)"""
    mu = _mu(codes, s, b0[:, None], b1[:, None])[:, :, 0]
    w = mu * (1.0 + alpha[None] * c) / (1.0 + alpha[None] * mu) ** 2
    return w[codes == 0].sum(axis=0), w[codes == 1].sum(axis=0)


def beta1_of(far_end, S, t):
    return np.where(far_end >= 0, S, -S)[:, None] * np.sinh(t) if np.ndim(t) == 2 else np.where(far_end >= 0, S, -S) * np.sinh(t)


def t_of(b1, S):
    return np.arcsinh(np.abs(b1) / S)


def far_end(q, flags):
    """sg E from K22's group fits (q, flags; G x 2): E = |log q1 - log q0| + 1, or 30 where a group is floored"""
    mle = np.log(q[:, 1]) - np.log(q[:, 0])
    E = np.where(((flags & FLOORED) != 0).any(axis=1), FAR_FLOORED, np.abs(mle) + 1.0)
    return np.where(mle >= 0, E, -E)


def search(counts, codes, s, alpha, far, S, sigma0=SIGMA0, chunk=64):
    """the maximiser BY DEFINITION: six rounds of the 64-point grid t_i = lo + (hi - lo) i / 63 from [0, asinh(E / S)] on
    t -> p(sg S sinh t); the first largest value at b; the next bracket [t_max(b-1,0), t_min(b+1,63)].  Returns a dict of (G,)
    arrays: b0, b1, p, t, w0, w1, flags.  A NaN alpha gives NaN and no flags."""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    G = c.shape[1]
    alpha, far = np.asarray(alpha, dtype=np.float64), np.asarray(far, dtype=np.float64)
    out = {k: np.full(G, np.nan) for k in ("b0", "b1", "p", "t", "w0", "w1")}
    out["flags"] = np.zeros(G, dtype=np.int32)
    live = np.flatnonzero(~np.isnan(alpha))
    i = np.arange(GRID, dtype=np.float64)
    for at in range(0, live.size, chunk):
        j = live[at:at + chunk]
        cj, aj, fj = c[:, j], alpha[j], far[j]
        rows = np.arange(j.size)
        lo, hi = np.zeros(j.size), np.arcsinh(np.abs(fj) / S)
        at_end = np.ones(j.size, dtype=bool)
        for r in range(ROUNDS):
            t = lo[:, None] + (hi - lo)[:, None] * i / 63.0
            b1 = beta1_of(fj, S, t)
            p, b0 = profile(cj, codes, s, aj, b1, S, sigma0)
            b = np.argmax(p, axis=1)
            out["flags"][j] |= np.where(at_end & (b == GRID - 1), AT_BOUND, 0).astype(np.int32)
            at_end &= b == GRID - 1
            lo, hi = t[rows, np.maximum(b - 1, 0)], t[rows, np.minimum(b + 1, GRID - 1)]
        out["b0"][j], out["b1"][j], out["p"][j], out["t"][j] = b0[rows, b], b1[rows, b], p[rows, b], t[rows, b]
        out["w0"][j], out["w1"][j] = weights(cj, codes, s, aj, out["b0"][j], out["b1"][j])
    return out


def bound(c, codes, s, alpha, b0, b1, S, sigma0=SIGMA0):
    """B of the parity rule: 64 ulp of the magnitudes actually added"""
    m = c.shape[0]
    mag = sum(np.abs(t).sum(axis=0) for t in likelihood_terms(c, codes, s, alpha, b0, b1))[:, 0]
    return 64 * 2.0 ** -53 * (mag + b0 ** 2 / (2.0 * sigma0 ** 2) + np.log1p((b1 / S) ** 2) + 4 * m + 2)


def resolved(c, codes, s, alpha, far, S, found, delta=1e-4, sigma0=SIGMA0):
    """the genes whose maximiser is pinned: the winner is not lane 0 or 63 of the first bracket (t -+ delta lie inside
    [0, asinh(E / S)]), and p drops by more than 2 B at t -+ delta.  found: the dict of search()."""
    out = np.zeros(alpha.size, dtype=bool)
    j = np.flatnonzero(~np.isnan(alpha))
    cj, aj, fj = c[:, j], alpha[j], far[j]
    t = found["t"][j]
    ts = np.stack([t - delta, t, t + delta], axis=1)
    p, _ = profile(cj, codes, s, aj, beta1_of(fj, S, ts), S, sigma0)
    B = bound(cj, codes, s, aj, found["b0"][j], found["b1"][j], S, sigma0)
    inner = (t - delta > 0.0) & (t + delta < np.arcsinh(np.abs(fj) / S))
    out[j] = inner & (p[:, 1] - p[:, 0] > 2 * B) & (p[:, 1] - p[:, 2] > 2 * B)
    return out


def prior_scale(lfc, se, use=None):
    """(S, A): A the root on [1e-6, 400] of f(A) = sum (D^2 - V - A) / (V + A)^2 over the usable genes (D = lfc, V = se^2), the
    score of the marginal likelihood D ~ N(0, V + A); the ends where f does not change sign; S = min(sqrt(A), 1)"""
    D, V = np.asarray(lfc, dtype=np.float64), np.asarray(se, dtype=np.float64) ** 2
    ok = np.isfinite(D) & np.isfinite(V)
    if use is not None:
        ok &= np.asarray(use, dtype=bool)
    D, V = D[ok], V[ok]
    f = lambda A: float(((D * D - V - A) / (V + A) ** 2).sum())
    if f(1e-6) <= 0:
        A = 1e-6
    elif f(400.0) >= 0:
        A = 400.0
    else:
        A = optimize.brentq(f, 1e-6, 400.0, xtol=1e-14, rtol=1e-14, maxiter=500)
    return min(np.sqrt(A), 1.0), A


def posterior_sd(b1, w0, w1, S, sigma0=SIGMA0):
    """the Laplace approximation of the posterior standard deviation of b1: from the Hessian of -P in (b0, b1)"""
    h00 = w0 + w1 + 1.0 / sigma0 ** 2
    h11 = w1 + 2.0 * (S * S - b1 * b1) / (S * S + b1 * b1) ** 2
    det = h00 * h11 - w1 * w1
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(det > 0, np.sqrt(h00 / det), np.nan)


# ---- the gene classes of the tests ------------------------------------------------------------------------------------------------
def two_maxima(c, codes, s, alpha, far, S, points=400):
    """per gene whether p has two local maxima on a dense grid of t over [0, asinh(|far| / S)] (an end point counts)"""
    G = c.shape[1]
    t = np.arcsinh(np.abs(far) / S)[:, None] * np.arange(points) / (points - 1.0)
    p, _ = profile(c, codes, s, alpha, beta1_of(far, S, t), S)
    pad = np.concatenate([np.full((G, 1), -np.inf), p, np.full((G, 1), -np.inf)], axis=1)
    peaks = (pad[:, 1:-1] > pad[:, :-2]) & (pad[:, 1:-1] >= pad[:, 2:])
    return peaks.sum(axis=1) >= 2


def bimodal_pair(s, codes, S, seed=23, tries=240):
    """two genes (m, 2) of the NB generator with a fold change whose profile has two local maxima at prior scale S: in the first
    the maximum next to 0 wins, in the second the one next to the MLE.  Also returns whether both were found (else the columns
    are plain genes of the same generator)."""
    rng = np.random.default_rng(seed)
    base = np.exp(rng.uniform(np.log(5.0), np.log(300.0), tries))
    fold = np.exp(rng.uniform(0.4, 1.6, tries) * rng.choice([-1.0, 1.0], tries))
    a = 0.05 + 2.0 / base
    mean = s[:, None] * base[None] * np.where(codes == 1, 1.0, 0.0)[:, None] * (fold[None] - 1.0) + s[:, None] * base[None]
    c = RR.nb_counts(rng, mean, a[None])
    q, _, flags = RR.group_fits(c, codes, 2, s, a)
    far = far_end(q, flags)
    two = two_maxima(c, codes, s, a, far, S) & ~(flags != 0).any(axis=1)
    found = search(c, codes, s, a, far, S)
    mle = np.abs(np.log(q[:, 1]) - np.log(q[:, 0]))
    near, away = np.flatnonzero(two & (np.abs(found["b1"]) < S)), np.flatnonzero(two & (np.abs(found["b1"]) > 0.5 * mle))
    ok = bool(near.size and away.size)
    pick = [near[0], away[0]] if ok else [0, 1]
    return c[:, pick], a[pick], ok
