"""numpy statement of the Cook's-distance rule of DESIGN.md K25 (pilot_ot_nb_cooks), the replacement rule and the independent
filtering of engine.independent_filtering, each by ANOTHER ROUTE than the product's: np.sort per group and math.fsum where the
device runs a bitonic network and a butterfly; the hat diagonal from the explicit m x k design,
diag(W^1/2 X (X'WX)^-1 X' W^1/2), where the device divides a weight by its group's sum; plain Python loops for Benjamini-Hochberg,
lowess and the filter where the product is vectorised.  Not collected by pytest (no test_ prefix).  The gene classes of the GPU
tests live here too, with the two conditions the tests' exact comparisons rest on (no distance next to the cutoff, no
replacement next to an integer), checked HERE, on this restatement, when a case is built."""
import math
from fractions import Fraction

import numpy as np
from scipy import stats

import nb_glm_restatement as RR

MIN_MU = 0.5
MIN_ROBUST_DISP = 0.04
MIN_GROUP = 3
MIN_REPLACE = 7
BASE_TRIM = Fraction(1, 5)


def trim_rule(n):
    """(trim ratio, scale) of a group of n samples"""
    if n <= 3:
        return Fraction(1, 3), 2.04
    if n <= 23:
        return Fraction(1, 4), 1.86
    return Fraction(1, 8), 1.51


def tm(x, r):
    """R's mean(x, trim = r): without the floor(n r) lowest and highest values (r exact, a Fraction or a float)"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    d = int(math.floor(x.size * Fraction(r)))
    kept = x[d:x.size - d]
    return math.fsum(kept) / kept.size


def cutoff(m, p):
    return float(stats.f.ppf(0.99, p, m - p))


def hat_diagonal(w, codes, k):
    """diag(W^1/2 X (X' W X)^-1 X' W^1/2) of the m x k indicator design"""
    X = np.zeros((w.size, k))
    X[np.arange(w.size), codes] = 1.0
    A = np.sqrt(w)[:, None] * X
    return ((A @ np.linalg.inv(X.T @ (w[:, None] * X))) * A).sum(axis=1)


def cooks(counts, codes, k, s, alpha, q, cut, min_replace=MIN_REPLACE):
    """dict of per-gene arrays as engine.nb_cooks returns them, with D (m x G) and D_scale: the same expression with |c - mu|
    replaced by c + mu, what the subtraction's rounding is measured against"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    m, G = c.shape
    codes = np.asarray(codes)
    size = np.bincount(codes, minlength=k)
    n_of = size[codes]
    out = {name: np.full(G, np.nan) for name in ("alpha_robust", "max_cooks", "trimmed_base")}
    out["arg_max"] = np.full(G, -1, dtype=np.int32)
    out["n_above"], out["n_replace"] = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    D, scale_of = np.full((m, G), np.nan), np.full((m, G), np.nan)
    big = [g for g in range(k) if size[g] >= MIN_GROUP]
    for j in range(G):
        cj, a = c[:, j], alpha[j]
        if np.isnan(a) or not cj.any():
            continue
        qj = cj / s
        out["trimmed_base"][j] = tm(qj, BASE_TRIM)
        if not big:
            continue
        v = []
        for g in big:
            r, scale = trim_rule(size[g])
            x = qj[codes == g]
            v.append(scale * tm((x - tm(x, r)) ** 2, r))
        mean_q = math.fsum(qj) / m
        a_rob = max((max(v) - mean_q) / mean_q ** 2, MIN_ROBUST_DISP)
        mu = np.maximum(s * q[j, codes], MIN_MU)
        with np.errstate(divide="ignore", invalid="ignore"):
            h = hat_diagonal(mu / (1.0 + a * mu), codes, k)
            tail = h / (k * (1.0 - h) ** 2) / (mu + a_rob * mu * mu)
            d, d_scale = (cj - mu) ** 2 * tail, (cj + mu) ** 2 * tail
        d[n_of == 1], d_scale[n_of == 1] = np.nan, np.nan
        D[:, j], scale_of[:, j] = d, d_scale
        elig = n_of >= MIN_GROUP
        top = d[elig].max()
        at = int(np.flatnonzero(elig & (d == top))[0])
        out["alpha_robust"][j], out["max_cooks"][j], out["arg_max"][j] = a_rob, top, at
        out["n_above"][j] = np.count_nonzero(cj > cj[at])
        with np.errstate(invalid="ignore"):
            out["n_replace"][j] = np.count_nonzero((d > cut) & (n_of >= min_replace))
    out["D"], out["D_scale"] = D, scale_of
    return out


def replacements(counts, codes, s, D, cut, trimmed_base, min_replace=MIN_REPLACE):
    """[(gene, sample, count, replacement)] by gene, then sample; replacement = trunc(trimmed_base s_j), R's as.integer"""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    n_of = np.bincount(codes)[codes]
    rows = []
    for j in range(c.shape[1]):
        for i in range(c.shape[0]):
            if n_of[i] >= min_replace and D[i, j] > cut:
                rows.append((j, i, c[i, j], float(math.trunc(trimmed_base[j] * s[i]))))
    return rows


def refit_max_cooks(new, codes, D, min_replace=MIN_REPLACE):
    """(maxCooks, n_above) of refitted genes: over the samples of groups with 3 <= n_g < min_replace only"""
    n_of = np.bincount(codes)[codes]
    G = new.shape[1]
    mc, na = np.full(G, np.nan), np.zeros(G, dtype=np.int32)
    for j in range(G):
        best = None
        for i in range(new.shape[0]):
            if MIN_GROUP <= n_of[i] < min_replace and not np.isnan(D[i, j]) and (best is None or D[i, j] > D[best, j]):
                best = i
        if best is not None:
            mc[j], na[j] = D[best, j], sum(1 for i in range(new.shape[0]) if new[i, j] > new[best, j])
    return mc, na


# ---- Benjamini-Hochberg, lowess and the filter as loops -----------------------------------------------------------------------------
def bh(p):
    p = [float(v) for v in p]
    n = len(p)
    order = sorted(range(n), key=lambda i: p[i])                       # (stable)
    out, running = [0.0] * n, 1.0
    for rank in range(n, 0, -1):
        i = order[rank - 1]
        running = min(running, p[i] * n / rank)
        out[i] = running
    return np.array(out)


def lowess(x, y, f, iters=3):
    x, y = [float(v) for v in x], [float(v) for v in y]
    n = len(x)
    ns = max(min(n, int(f * n + 1e-7)), 2)
    rw, fit = [1.0] * n, [0.0] * n
    for it in range(iters + 1):
        nleft, nright = 0, ns - 1
        for i in range(n):
            while nright < n - 1 and x[nright + 1] - x[i] < x[i] - x[nleft]:
                nleft += 1
                nright += 1
            h = max(x[i] - x[nleft], x[nright] - x[i])
            w, js = [], []
            for j in range(nleft, n):
                r = abs(x[j] - x[i])
                if r <= 0.999 * h:
                    w.append((1.0 if r <= 0.001 * h else (1.0 - (r / h) ** 3) ** 3) * rw[j])
                    js.append(j)
                elif x[j] > x[i]:
                    break
            a = sum(w)
            if not a > 0:
                fit[i] = y[i]
                continue
            w = [v / a for v in w]
            if h > 0:
                centre = sum(v * x[j] for v, j in zip(w, js))
                c = sum(v * (x[j] - centre) ** 2 for v, j in zip(w, js))
                if math.sqrt(c) > 0.001 * (x[-1] - x[0]):
                    b = (x[i] - centre) / c
                    w = [v * (b * (x[j] - centre) + 1.0) for v, j in zip(w, js)]
            fit[i] = sum(v * y[j] for v, j in zip(w, js))
        if it == iters:
            break
        res = [abs(y[i] - fit[i]) for i in range(n)]
        part = sorted(res)
        cmad = 3.0 * (part[n // 2] + part[n - n // 2 - 1])
        if cmad < 1e-7 * (sum(res) / n):
            break
        rw = [1.0 if r <= 0.001 * cmad else ((1.0 - (r / cmad) ** 2) ** 2 if r <= 0.999 * cmad else 0.0) for r in res]
    return np.array(fit)


def independent_filtering(pvalue, base_mean, alpha, fit_lowess=lowess):
    p = np.asarray(pvalue, dtype=np.float64)
    filt = np.array([0.0 if np.isnan(v) else v for v in base_mean])
    lo = float(np.mean(filt == 0))
    theta = np.linspace(lo, 0.95, 50) if lo < 0.95 else np.zeros(1)
    columns, num_rej, cuts = [], [], []
    for t in theta:
        cut = np.quantile(filt, t)
        col = np.full(p.size, np.nan)
        use = [i for i in range(p.size) if filt[i] >= cut and not np.isnan(p[i])]
        if use:
            col[use] = bh(p[use])
        columns.append(col)
        cuts.append(float(cut))
        num_rej.append(sum(1 for v in col if v < alpha))
    chosen, fit = 0, None
    if max(num_rej) > 10:
        fit = fit_lowess(theta, num_rej, 0.2)
        res = [num_rej[i] - fit[i] for i in range(len(num_rej)) if num_rej[i] > 0]
        thresh = max(fit) - math.sqrt(sum(r * r for r in res) / len(res))
        for i, n in enumerate(num_rej):
            if n > thresh:
                chosen = i
                break
    return columns[chosen], {"theta": theta, "num_rej": np.array(num_rej, dtype=np.int64), "lowess": fit, "chosen": chosen,
                             "filter_threshold": cuts[chosen]}


# ---- the gene classes of the tests ---------------------------------------------------------------------------------------------------
CLASSES = ("clean", "outlier in a replaceable group", "outlier in a flaggable group", "planted zero", "two outliers", "single count",
           "tied", "zeros", "nan dispersion")


def tied_size_factors(rng, m):
    """K22's size factors with every third one set to 1, so that equal counts give equal c / s"""
    s = RR.size_factors(rng, m)
    s[::3] = 1.0
    return s


def _one_gene(rng, s, codes, k, kind):
    """(counts of one gene, its dispersion)"""
    m = s.size
    size = np.bincount(codes, minlength=k)
    c = RR.nb_class(rng, s, codes, k, 1)[:, 0]
    alpha = float(np.clip(0.05 + 2.0 / max(c.mean(), 1.0), RR.MIN_DISP, RR.max_disp(m)))
    name = CLASSES[kind]

    def member(ok):
        groups = np.flatnonzero(ok)
        return None if groups.size == 0 else int(rng.choice(np.flatnonzero(codes == rng.choice(groups))))

    if name.startswith("outlier") or name == "two outliers":
        c = np.maximum(c, 5.0)
        ok = size >= MIN_REPLACE if name != "outlier in a flaggable group" else (size >= MIN_GROUP) & (size < MIN_REPLACE)
        for _ in range(2 if name == "two outliers" else 1):
            i = member(ok if ok.any() else size >= 1)
            c[i] = c[i] * 200.0
    elif name == "planted zero":
        c = np.rint(s * 1000.0 * np.exp(rng.normal(0.0, 0.05, m)))
        c[member(size >= 1)] = 0.0
        alpha = 0.05
    elif name == "single count":
        c = np.zeros(m)
        c[member(size >= 1)] = float(rng.integers(20, 400))
        alpha = 1.0
    elif name == "tied":
        c = np.full(m, float(rng.integers(3, 60)))
        c[rng.random(m) < 0.3] = 0.0
        c[0] = max(c[0], 4.0)
        alpha = 0.2
    elif name == "zeros":
        c = np.zeros(m)
    elif name == "nan dispersion":
        alpha = np.nan
    return c, alpha


def conditions_hold(want, s, cut):
    """per gene: no D_j and no max_cooks within 1e-6 relative of the cutoff, no trimmed_base s_j within 1e-9 of an integer (an
    exact 0, the trimmed mean of zeros, is exact on every route and allowed)"""
    D, base = want["D"], want["trimmed_base"]
    with np.errstate(invalid="ignore"):
        near = (np.abs(D - cut) <= 1e-6 * cut).any(axis=0) | (np.abs(want["max_cooks"] - cut) <= 1e-6 * cut)
        x = base[None] * s[:, None]
        near |= ((np.abs(x - np.rint(x)) <= 1e-9) & (x != 0)).any(axis=0)
    return ~near


def case(seed, sizes, G, min_replace=MIN_REPLACE):
    """one test case: the samples of `sizes` in a shuffled order, G genes cycling through the classes, the dispersions, the group
    fits (K22's restatement) and the restatement's answer; a gene that breaks a condition is drawn again (clean class)"""
    rng = np.random.default_rng(seed)
    k, m = len(sizes), int(sum(sizes))
    codes = rng.permutation(np.repeat(np.arange(k), sizes)).astype(np.int32)
    s = tied_size_factors(rng, m)
    cut = cutoff(m, k)
    kind = np.arange(G) % len(CLASSES) if G > 2 else np.array([1, 0])[:G]
    c, alpha = np.zeros((m, G)), np.zeros(G)
    for j in range(G):
        c[:, j], alpha[j] = _one_gene(rng, s, codes, k, kind[j])
    for _ in range(20):
        q = RR.group_fits(c, codes, k, s, alpha)[0]
        want = cooks(c, codes, k, s, alpha, q, cut, min_replace)
        bad = np.flatnonzero(~conditions_hold(want, s, cut))
        if bad.size == 0:
            break
        for j in bad:
            kind[j] = 0
            c[:, j], alpha[j] = _one_gene(rng, s, codes, k, 0)
    assert conditions_hold(want, s, cut).all()
    out = dict(m=m, k=k, G=G, sizes=tuple(sizes), codes=codes, s=s, c=c, alpha=alpha, q=q, cutoff=cut, kind=kind, want=want,
               min_replace=min_replace)
    for a in (codes, s, c, alpha, q, kind, want["D"], want["D_scale"]):
        a.flags.writeable = False
    return out
