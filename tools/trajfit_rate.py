#!/usr/bin/env python3
"""Wall time of the trajectory model fits (engine.trajectory_fits: pilotpy's fit_best_model with LinearRegression, and with
HuberRegressor on log1p of the same counts) against a reference-style CPU loop (per target: the scikit-learn regressor for each
of the three models, the numpy p-values of fit_model_activity, the per-observation modified-R^2 loop, scipy's pearsonr), at
(n, targets) = (634, 14), (5000, 2000) and (20000, 20000), float32 counts-like targets, time = sample rank.

The device time is the whole call from a host array (upload included) and from a DeviceMatrix already in HBM.  The CPU loop runs
on at most --cpu-targets targets and is reported per target and extrapolated to all of them.  Writes
profiles/trajfit/trajfit_rate.txt.  GPU only."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pilot_amd import _lib, engine  # noqa: E402

SHAPES = [(634, 14), (5000, 2000), (20000, 20000)]


def make(n, T, seed=0):
    rng = np.random.default_rng(seed)
    n_samples = max(n // 25, 10)
    x = np.sort(rng.integers(1, n_samples + 1, n)).astype(np.float64)
    lam = rng.gamma(0.3, 1.0, T).astype(np.float32)[None, :] * (1 + (x / n_samples).astype(np.float32)[:, None])
    return x, rng.poisson(lam).astype(np.float32)


def reference_style(x, y, huber=False):
    """fit_best_model's per-target work as the reference does it (restated here, CPU)"""
    import warnings
    from scipy import stats
    warnings.simplefilter("ignore")
    from sklearn.linear_model import HuberRegressor, LinearRegression
    for f in ([x], [x, x * x], [x * x]):
        X = np.column_stack(f)
        model = (HuberRegressor(epsilon=1.35) if huber else LinearRegression()).fit(X, y)
        params = np.append(model.intercept_, model.coef_)
        pred = model.predict(X)
        model.score(X, y)
        msse = 0.0
        for e in y - pred:
            msse += 0.5 * e * e if abs(e) < 1.35 else 1.35 * (abs(e) - 0.675)
        Z = np.append(np.ones((len(X), 1)), X, axis=1)
        mse = np.sum((y - pred) ** 2) / (len(Z) - len(Z[0]))
        se = np.sqrt(mse * np.linalg.inv(Z.T @ Z).diagonal())
        [2 * (1 - stats.t.cdf(abs(t), len(Z) - len(Z[0]))) for t in params / se]
    stats.pearsonr(x, y)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-targets", type=int, default=14)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajfit", "trajfit_rate.txt"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("trajfit_rate.py needs a HIP device")
    lines = ["# trajectory model fits, float32 targets (huber: log1p of the counts); device: %s" % _lib.device_name(),
             "# model n targets | device ms (host array) | device ms (DeviceMatrix) | GB read per pass | CPU loop ms/target | CPU loop s (all, extrapolated) | speed-up (host array)"]
    for model in ("ols", "huber"):
        for n, T in SHAPES:
            x, Y = make(n, T)
            if model == "huber":
                Y = np.log1p(Y)
            reps = 5 if n * T < 1e8 else 3
            t_host = timed(lambda: engine.trajectory_fits(Y, x, model=model), reps)
            D = engine.DeviceMatrix.upload(Y)
            t_dev = timed(lambda: engine.trajectory_fits(D, x, model=model), reps)
            del D
            k = min(T, args.cpu_targets)
            t0 = time.perf_counter()
            for j in range(k):
                reference_style(x, Y[:, j].astype(np.float64), huber=model == "huber")
            cpu = 1e3 * (time.perf_counter() - t0) / k
            line = "%-5s %6d %6d | %10.2f | %10.2f | %6.3f | %8.1f | %10.1f | %8.0fx" % (
                model, n, T, t_host, t_dev, Y.nbytes / 1e9, cpu, cpu * T / 1e3, cpu * T / t_host)
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
