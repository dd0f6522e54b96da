#!/usr/bin/env python3
"""Time of the negative-binomial GLM kernels (K22: engine.nb_dispersions, engine.nb_group_fits) beside the vectorised numpy /
scipy restatement (tests/nb_glm_restatement.py) on the same host.

Table: genes x samples of the tests' NB generator (base mean log-uniform on [2, 3000], alpha = 0.05 + 2 / base, 20 % fold
changes), two groups of m / 2 samples, float32 in HBM (a DeviceMatrix), at --samples sizes (default 24 and 600) and --genes
(default 20 000).  Per size, after one warm-up call of each, the host clock around ``nb_dispersions`` (gene-wise, then with a
prior: the MAP pass) and around ``nb_group_fits`` -- each call ends in device-to-host copies of its results -- best of --reps.
``lgamma-free``: the same call on a table of the same shape whose counts are zero but for one sample a gene; there the kernel takes
its c = 0 path for all but one sample (log1p, one division and the running sums: everything it does except the two lgamma and the
log of a positive count), which prices the arithmetic around lgamma.  Host: the restatement on --host-genes of the genes (default
200), scaled by genes / host-genes and reported as such.  No DESeq2 timing exists where this library is built.
Writes OUT/rate.txt (--out, default profiles/pseudobulk_de/)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudobulk_de"))
    ap.add_argument("--samples", type=int, nargs="+", default=[24, 600])
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--host-genes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import nb_glm_restatement as RR
    from pilot_amd import _lib, engine

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def best_of(fn):
        fn()
        best = np.inf
        for _ in range(a.reps):
            t = time.perf_counter()
            out = fn()
            best = min(best, time.perf_counter() - t)
        return best, out

    say("%s; %s; at most %d samples a gene" % (_lib.device_name(), time.strftime("%Y-%m-%d"), engine.nb_glm_limits()))
    for m in a.samples:
        rng = np.random.default_rng(m)
        s = RR.size_factors(rng, m)
        codes = (np.arange(m) % 2).astype(np.int32)
        c = RR.nb_class(rng, s, codes, 2, a.genes)
        D = engine.DeviceMatrix.upload(c.astype(np.float32))
        t_gene, x = best_of(lambda: engine.nb_dispersions(D, codes, 2, s))
        prior = np.log(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1e-3))
        t_map, x_map = best_of(lambda: engine.nb_dispersions(D, codes, 2, s, log_prior_mean=prior, prior_var=0.6))
        alpha = engine.nb_clip(np.exp(x_map), m)
        t_fit, fits = best_of(lambda: engine.nb_group_fits(D, codes, 2, s, alpha, return_info=True))
        sparse = np.zeros((m, a.genes), dtype=np.float32)
        sparse[rng.integers(0, m, a.genes), np.arange(a.genes)] = 1.0 + rng.integers(0, 40, a.genes)
        Z = engine.DeviceMatrix.upload(sparse)
        t_free, _ = best_of(lambda: engine.nb_dispersions(Z, codes, 2, s))
        say("case %d genes x %d samples, float32 in HBM, 2 groups" % (a.genes, m))
        say("  nb_dispersions %.2f ms gene-wise, %.2f ms with the prior; nb_group_fits %.2f ms (at most %d steps, %d not converged); "
            "best of %d" % (1e3 * t_gene, 1e3 * t_map, 1e3 * t_fit, fits[2]["steps"].max(), fits[2]["n_not_converged"], a.reps))
        evals = a.genes * m * 64.0 * 6
        say("  %.3g likelihood terms a call: %.1f ps a term on the whole device; lgamma-free table %.2f ms: the "
            "full call is %.1f x it" % (evals, 1e12 * t_gene / evals, 1e3 * t_free, t_gene / t_free))
        h = min(a.host_genes, a.genes)
        t0 = time.perf_counter()
        xh = RR.dispersions(c[:, :h], codes, 2, s)[0]
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        RR.group_fits(c[:, :h], codes, 2, s, np.exp(xh))
        t_host_fit = time.perf_counter() - t0
        res = RR.resolved(c[:, :h], RR.fitted_mu(c[:, :h], codes, 2, s), codes, 2, xh)
        say("  host restatement on %d genes: dispersions %.2f s, group fits (200 bisection steps) %.2f s; scaled by %d / %d: %.0f s and "
            "%.0f s; device against it on the resolved genes (%d): dispersion off by at most %.2g relative"
            % (h, t_host, t_host_fit, a.genes, h, t_host * a.genes / h, t_host_fit * a.genes / h, res.sum(),
               np.abs(np.expm1(x[:h][res] - xh[res])).max(initial=0)))
        del D, Z
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
