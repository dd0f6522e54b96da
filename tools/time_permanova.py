#!/usr/bin/env python3
"""Time of PERMANOVA on the device (K29, engine.permanova_ss) beside the numpy loop on the same host.

Cases: --samples (default 600 and 2000) Euclidean distances of seeded points plus an asymmetric perturbation, uploaded once as an
``engine.DeviceMatrix``; a 3-level term (c = 2 columns) and a batch of 4 terms (c = 8: 3, 4, 2 and 3 levels); --permutations (default 99 999).  Device: the host clock around ``permanova_ss`` (it ends in
device-to-host copies) after one warm-up call, best of --reps; then one more call with ``return_times=True`` for the device
milliseconds of the prepare, permute and quadratic-form kernels (events on the launch stream around each kernel group, the
library's own hook; that call synchronises after every group and is not the one timed).  Floor: ``2 n^2 c (permutations + 1)``
flop at the f64 matrix rate, --peak-tflops (default 78.6, the datasheet figure SURVEY.md quotes; it is not measured here); the
ratio quoted is quadratic-form kernel time over that floor.  Host (--host-permutations, default 200, scaled to the device's
count): per permutation ``Z = Q[rng.permutation(n)]`` and per term ``(Z * (A @ Z)).sum()`` in float64 numpy.
Writes OUT/permanova_rate.txt (--out, default profiles/permanova/)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def distances(n, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, 8)
    G = X @ X.T
    d2 = np.maximum(np.diag(G)[:, None] + np.diag(G)[None, :] - 2 * G, 0.0)
    return np.sqrt(d2) + 0.05 * rs.rand(n, n) + 0.01


def design(n, batch, seed):
    rs = np.random.RandomState(seed)
    level = lambda k: np.array(["l%d" % i for i in range(k)], dtype=object)[rs.randint(0, k, n)]
    if not batch:
        return {"three": level(3)}
    return {"three": level(3), "four": level(4), "two": level(2), "other": level(3)}


def host_loop(A, Q, terms, count, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((count, len(terms) - 1))
    t0 = time.perf_counter()
    for b in range(count):
        Z = Q[rng.permutation(Q.shape[0])]
        T = Z * (A @ Z)
        out[b] = [T[:, terms[t]:terms[t + 1]].sum() for t in range(len(terms) - 1)]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permanova"))
    ap.add_argument("--samples", type=int, nargs="+", default=[600, 2000])
    ap.add_argument("--permutations", type=int, default=99999)
    ap.add_argument("--host-permutations", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    a = ap.parse_args()
    from pilot_amd import _lib, engine

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("PERMANOVA (K29) on %s, %d permutations + the observed design, best of %d; limits %s; floor at %.1f TF f64 matrix (datasheet, "
        "not measured)" % (_lib.device_name(), a.permutations, a.reps, engine.permanova_limits(), a.peak_tflops))
    say("%7s %3s %6s | %9s %9s | %8s %8s %9s | %9s %7s | %11s %7s"
        % ("samples", "c", "terms", "call ms", "us/perm", "prepare", "permute", "quadratic", "floor ms", "x floor", "numpy s", "x numpy"))
    for n in a.samples:
        D = distances(n, n)
        dev = engine.DeviceMatrix.upload(D)
        S = (D + D.T) / 2
        np.fill_diagonal(S, 0.0)
        A = -0.5 * S * S
        for batch in (False, True):
            Q, terms = engine.permanova_basis(design(n, batch, n + 1))
            c = Q.shape[1]
            engine.permanova_ss(dev, Q, terms, a.permutations, seed=1)
            best = np.inf
            for _ in range(a.reps):
                t0 = time.perf_counter()
                engine.permanova_ss(dev, Q, terms, a.permutations, seed=1)
                best = min(best, time.perf_counter() - t0)
            ms = engine.permanova_ss(dev, Q, terms, a.permutations, seed=1, return_times=True)[2]
            floor_ms = 2.0 * n * n * c * (a.permutations + 1) / (a.peak_tflops * 1e12) * 1e3
            host = host_loop(A, Q, terms, a.host_permutations, 0) * (a.permutations + 1) / a.host_permutations
            say("%7d %3d %6d | %9.2f %9.3f | %8.3f %8.2f %9.2f | %9.2f %7.2f | %11.2f %7.0f"
                % (n, c, len(terms) - 1, best * 1e3, best * 1e6 / (a.permutations + 1), ms["prepare"], ms["permute"], ms["quadratic"],
                   floor_ms, ms["quadratic"] / floor_ms, host, host / best))
    say("call ms: host clock around engine.permanova_ss (D in HBM; Q up, SS back).  prepare / permute / quadratic: device ms of the kernel")
    say("groups in a separate call.  x floor: quadratic-form kernel time over 2 n^2 c permutations flop at the quoted rate.  numpy s: the")
    say("host loop on %d permutations scaled to %d." % (a.host_permutations, a.permutations + 1))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "permanova_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
