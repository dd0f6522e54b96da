#!/usr/bin/env python3
"""Rates of gene_cluster_differentiation's device part (K10, engine.bootstrap_huber_fits) and of its host draws, against a
reference-style CPU loop (one scikit-learn HuberRegressor fit per bootstrap, as Gene_cluster_specific.py runs them).

Cases: R rows x n cells (one cluster's log1p counts, f32, R gene columns; models cycling linear / linear_quadratic / quadratic;
B = 50 resamples each), and the mean-curve side (R rows of 20-point curves, x = pline).  Device time: host clock around the call
(it ends in a device-to-host copy), after a warm-up call of the same shape; the median of --reps.  Host draws: numpy's legacy
RandomState.randint, 50 per row.  The CPU loop fits --cpu-fits resamples of the largest case on one core and on --cpu-workers
processes, and is scaled to the case.  Prints one line per case and writes them to OUT/gene_cluster_rate.txt (--out, default
profiles/gene_cluster/)."""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "1")


def _case(rng, R, n, B=50):
    t = np.sort(rng.integers(1, 41, n)).astype(np.float64)
    lam = rng.gamma(0.8, 2.0, R)[None, :] * np.exp(np.outer(t / 40, rng.normal(0, 1.5, R)))
    Y = np.log1p(rng.poisson(lam)).astype(np.float32)
    idx = rng.integers(0, n, (R, n, B)).astype(np.int32)
    return Y, t, np.arange(R, dtype=np.int32), (np.arange(R) % 3).astype(np.int32), idx


def _sk_fits(args):
    from sklearn.linear_model import HuberRegressor
    x, y, model, idx = args
    for b in range(idx.shape[1]):
        xr = x[idx[:, b]]
        F = {0: xr[:, None], 1: np.column_stack((xr, xr * xr)), 2: (xr * xr)[:, None]}[model]
        HuberRegressor(epsilon=1.35).fit(F, y)
    return idx.shape[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gene_cluster"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-fits", type=int, default=48)
    ap.add_argument("--cpu-workers", type=int, default=16)
    ap.add_argument("--cases", default="200x3000,2000x3000,2000x20")
    a = ap.parse_args()
    from pilot_amd import engine
    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(0)
    lines = []
    for case in a.cases.split(","):
        R, n = (int(v) for v in case.split("x"))
        Y, t, cols, models, idx = _case(rng, R, n)
        if n == 20:                                            # the mean-curve side: x = pline, Y = the curves
            t = np.linspace(1, 40, 20)
        engine.bootstrap_huber_fits(Y, t, cols, models, idx)   # warm-up
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, info = engine.bootstrap_huber_fits(Y, t, cols, models, idx, return_info=True)
            times.append(time.perf_counter() - t0)
        dev = float(np.median(times))
        rs = np.random.RandomState(1)
        t0 = time.perf_counter()
        for _ in range(R):
            for _ in range(50):
                rs.randint(0, n, n)
        draw = time.perf_counter() - t0
        fits = R * 50
        line = ("rows=%d cells=%d B=50: device %.4f s per call (%.2f us per fit, %.3g fits/s; not converged %d), "
                "host draws %.4f s" % (R, n, dev, dev / fits * 1e6, fits / dev, info["not_converged"], draw))
        print(line, flush=True)
        lines.append(line)
    # reference-style CPU loop on the last case with n = 3000 (or the largest n)
    Rn = [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",")]
    R, n = max(Rn, key=lambda c: (c[1], c[0]))
    Y, t, cols, models, idx = _case(np.random.default_rng(2), 3, n)
    k = a.cpu_fits
    per = k // 3
    jobs = [(t, Y[:, q].astype(np.float64), int(models[q]), idx[q][:, :per]) for q in range(3)]
    t0 = time.perf_counter()
    for j in jobs:
        _sk_fits(j)
    one = (time.perf_counter() - t0) / (3 * per)
    chunks = [(t, Y[:, q % 3].astype(np.float64), q % 3, idx[q % 3][:, :per]) for q in range(a.cpu_workers)]
    with ProcessPoolExecutor(a.cpu_workers) as ex:
        list(ex.map(_sk_fits, chunks[:2]))                      # workers up
        t0 = time.perf_counter()
        done = sum(ex.map(_sk_fits, chunks))
        many = (time.perf_counter() - t0) / done
    line = ("CPU loop (scikit-learn HuberRegressor, n=%d): %.2f ms per fit on one core, %.3f ms per fit over %d processes; "
            "scaled to rows=%d x 50 fits: %.1f s / %.1f s"
            % (n, one * 1e3, many * 1e3, a.cpu_workers, R, one * R * 50, many * R * 50))
    print(line, flush=True)
    lines.append(line)
    with open(os.path.join(a.out, "gene_cluster_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
