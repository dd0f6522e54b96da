"""The numerical core of pilotpy's genes_selection_analysis restated on arrays with the libraries the reference calls
(plot/gene_selection_analysis.py:52-203, 352-415; plot/curve_activity.py): pandas' ``groupby(...).std()``, scikit-learn's
``StandardScaler``, scipy's ``pdist`` / ``linkage`` / ``fcluster`` / ``zscore`` / ``norm.sf``.  CPU only.  This, and through the
fixture tests/golden/gene_curves_*.npz the reference itself, is the yardstick of the K11 tests; nothing here touches the engine."""
import numpy as np
import pandas as pd
import scipy.cluster.hierarchy as sch
from scipy.stats import norm, zscore
from sklearn.preprocessing import StandardScaler

MODELS = ("linear", "linear_quadratic", "quadratic")


def design(func_type, x):
    """generate_feature_list"""
    x = np.asarray(x, dtype=np.float64)
    if func_type == "linear":
        return np.column_stack((np.ones(len(x)), x))
    if func_type == "linear_quadratic":
        return np.column_stack((np.ones(len(x)), x, np.power(x, 2)))
    assert func_type == "quadratic", func_type
    return np.column_stack((np.ones(len(x)), np.power(x, 2)))


def make_curves(params, models, times):
    """make_curves: params G x 3 (Intercept, Treat, Treat2), models: names"""
    out = np.empty((len(models), len(times)))
    for g, f in enumerate(models):
        coefs = np.array(params[g, :3] if f == "linear_quadratic" else params[g, :2], dtype=float)
        out[g] = np.matmul(design(f, times), coefs)
    return out


def segment_std(Y, cell_times):
    """(sorted unique times, T x columns): ``cells.groupby('Time_score').std()`` (ddof 1; one cell: NaN)"""
    df = pd.DataFrame(np.asarray(Y, dtype=np.float64))
    df["Time_score"] = np.asarray(cell_times)
    sd = df.groupby("Time_score").std()
    return sd.index.to_numpy(dtype=np.float64), sd.to_numpy()


def scale_rows(C):
    """StandardScaler over each row's values (fit_transform of the transpose, transposed back)"""
    if C.shape[0] == 0:
        return C.copy()
    return StandardScaler().fit_transform(C.T).T


def noised_curves(params, models, times, sd):
    """(scaled curves, scaled noised curves): sd is T x G; noise = sd / 10 * (Treat + Treat2 - Intercept), NaN -> 0"""
    curves = make_curves(params, models, times)
    sum_cov = np.sum(list(params[:, [1, 2, 0]] * [1, 1, -1]), axis=1) if len(models) else np.zeros(0)
    noise = pd.DataFrame(sd / 10).mul(sum_cov)
    noised = pd.DataFrame(curves) + noise.transpose()
    noised = noised.fillna(0).to_numpy()
    return scale_rows(curves), scale_rows(noised)


def select(table, feature="R-squared", pval="adjusted P-value", thr=0.1, pthr=0.05):
    table = table.fillna(0)
    return table[(np.abs(table[feature]) >= thr) & (table[pval] <= pthr)]


def linkage(curves, method="complete"):
    """(Z, d.max())"""
    d = sch.distance.pdist(curves)
    return sch.linkage(d, method=method, metric="correlation"), d.max()


def clusters(curves, method="complete", scaler_value=0.65):
    try:
        Z, dmax = linkage(curves, method)
        return sch.fcluster(Z, scaler_value * dmax, "distance")
    except ValueError:
        return np.ones(len(curves), dtype=np.int32)


def auc(curves, times):
    if len(times) < 2 or not (times[1:] > times[:-1]).all():
        raise ValueError("times must be increasing and have at least 2 values.")
    return ((curves[:, 1:] + curves[:, :-1]) / 2) @ (times[1:] - times[:-1])


def activities_raw(curves, times):
    """G x 4 unrounded: terminal logFC, transient logFC, switching time, area (curve_activity.py)"""
    curves, times = np.asarray(curves, dtype=np.float64), np.asarray(times, dtype=np.float64)
    if len(times) < 2 or not (times[1:] > times[:-1]).all():
        raise ValueError("times must be increasing and have at least 2 values.")
    n = curves.shape[1]
    terminal = (curves[:, -1] - curves[:, 0]) / (times[-1] - times[0])
    tn = (times - times[0]) / (times[-1] - times[0])
    med = np.median([curves, np.repeat(curves[:, [0]], n, axis=1), np.repeat(curves[:, [-1]], n, axis=1)], axis=0)
    transient = auc(curves - med, tn)
    switching = auc((med.T - med[:, -1]).T, tn) / (med[:, 0] - med[:, -1] + 1e-300)
    area = abs(curves[:, 0] + curves[:, -1]) * abs(times[-1] - times[0])
    return np.column_stack((terminal, transient, switching, area))


def adjust_p_values(p_values):
    p = np.asarray(p_values, dtype=np.float64)
    by_descend = p.argsort()[::-1]
    by_orig = by_descend.argsort()
    steps = float(len(p)) / np.arange(len(p), 0, -1)
    q = np.minimum(1, np.minimum.accumulate(steps * p[by_descend]))
    return q[by_orig]


def activities(curves, times, cluster_labels):
    """the frame of compute_curves_activities as a dict of columns"""
    raw = activities_raw(curves, times)
    tl = np.round(raw[:, 0], 2)
    p = norm.sf(abs(zscore(tl))) * 2
    return dict(Terminal_logFC=tl, Terminal_pvalue=p, Terminal_adjPvalue=adjust_p_values(p), Transient_logFC=np.round(raw[:, 1], 2),
                Switching_time=np.round(raw[:, 2], 2), area=np.round(raw[:, 3], 2), cluster=np.asarray(cluster_labels))


def rounding_margin(raw):
    """smallest distance of an unrounded value to a rounding boundary of np.round(., 2) (k + 0.5 hundredths)"""
    v = np.asarray(raw, dtype=np.float64) * 100.0
    return float(np.abs(v - np.floor(v) - 0.5).min() / 100.0)


def height_condition(Z, cut, rel=1e-9):
    """True when consecutive sorted heights all differ by more than ``rel`` relative and none lies within ``rel`` of the cut:
    the inputs on which Z's structure and the flat labels are compared exactly"""
    h = np.sort(Z[:, 2])
    gaps = np.diff(h) / h[1:] if h.size > 1 else np.array([np.inf])
    return bool(gaps.min() > rel and (np.abs(h - cut) / cut).min() > rel)


def merge_margins(curves, method="complete"):
    """Per merge of the restatement's Z: (m - h) / m, h the merge height and m the smallest distance from either merged cluster
    to any third cluster at that moment (inf when none is left).  A merge with a margin at rounding level is AMBIGUOUS: which
    partner a cluster takes is then decided by the last bits of its inputs, so scipy itself returns another tree, other cluster
    numbers and, above that height, another partition when its input moves by 1e-15 -- although every height stays where it
    was.  The standing example is a constant gene: its standardised row is 0, at distance sqrt(T) from EVERY other
    standardised row.  Replays the merges with the Lance-Williams update on the square matrix; scipy and numpy only."""
    curves = np.asarray(curves, dtype=np.float64)
    n = curves.shape[0]
    D = sch.distance.squareform(sch.distance.pdist(curves))
    np.fill_diagonal(D, np.inf)
    Z = sch.linkage(sch.distance.pdist(curves), method=method)
    slot = {i: i for i in range(n)}
    size = {i: 1 for i in range(n)}
    margins = np.full(n - 1, np.inf)
    for i in range(n - 1):
        ia, ib = int(Z[i, 0]), int(Z[i, 1])
        a, b = slot.pop(ia), slot.pop(ib)
        h = D[a, b]
        D[a, b] = D[b, a] = np.inf
        m = min(D[a].min(), D[b].min())
        if np.isfinite(m):
            margins[i] = (m - h) / m if m > 0 else 0.0
        na, nb = size.pop(ia), size.pop(ib)
        da, db = D[a], D[b]
        new = {"single": np.minimum(da, db), "complete": np.maximum(da, db), "average": (na * da + nb * db) / (na + nb),
               "weighted": 0.5 * (da + db)}[method]
        new[a] = new[b] = np.inf
        D[b, :] = new
        D[:, b] = new
        D[a, :] = np.inf
        D[:, a] = np.inf
        slot[n + i], size[n + i] = b, na + nb
    return Z, margins


def comparable(curves, method, cuts, rel=1e-9):
    """(exact, cuts whose partition is determined): ``exact`` when the issue's condition holds (:func:`height_condition` at every
    cut) AND no merge is ambiguous (:func:`merge_margins` all above ``rel``): then Z's structure, the sizes and the flat labels
    are compared exactly.  Otherwise only the sorted heights and, as labels up to a bijection, the partition at the cuts that lie
    below the lowest ambiguous merge (everything under it is still determined)."""
    Z, margins = merge_margins(curves, method)
    d = sch.distance.pdist(curves)
    bad = Z[margins <= rel, 2]
    exact = bad.size == 0 and all(height_condition(Z, c * d.max(), rel) for c in cuts)
    return exact, [c for c in cuts if bad.size == 0 or c * d.max() < bad.min() * (1 - rel)]


def same_partition(a, b):
    """labels equal up to a bijection"""
    a, b = np.asarray(a), np.asarray(b)
    fwd, back = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(x, y) != y or back.setdefault(y, x) != x:
            return False
    return True


def synthetic_table(rng, G, T):
    """(params G x 3, model names, times) of random fits of all three kinds over times 1..T: curves of O(1) size whose change
    over the time range is 0.3 .. 2 per term, so no curve is flat to rounding"""
    times = np.arange(1, T + 1, dtype=np.float64)
    names = np.asarray(MODELS)[rng.integers(0, 3, G)]
    mag = lambda: rng.choice([-1.0, 1.0], G) * rng.uniform(0.3, 2.0, G)
    params = np.column_stack((rng.normal(1.0, 0.5, G), mag() / T, mag() / T ** 2))
    quad = names == "quadratic"
    params[quad, 1] = mag()[quad] / T ** 2
    params[names != "linear_quadratic", 2] = 0.0
    return params, names, times


def synthetic_cells(rng, n_cells, T, n_genes, dtype=np.float64):
    """log-normalised-looking expression of n_cells over T time points (every time point has at least two cells), sorted by time"""
    t = np.sort(np.r_[np.repeat(np.arange(1, T + 1), 2), rng.integers(1, T + 1, n_cells - 2 * T)]).astype(np.float64)
    Y = np.log1p(rng.poisson(2.0, (n_cells, n_genes)) * rng.uniform(0.5, 2.0, (n_cells, 1))).astype(dtype)
    return Y, t
