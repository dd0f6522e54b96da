#!/usr/bin/env python3
"""Times of the gene curve clustering step (K11) on the device and of its restatement with pandas / scipy / scikit-learn
(tests/curves_restatement.py) on the same box's CPUs.

Cases G x T x cells: G selected genes, T time points, that many float32 cells with G gene columns (uniform values: the
arithmetic does not depend on them).  Device parts, each a host clock around a call that ends in a device-to-host copy or a
device synchronise, after a warm-up call of the same shape, the median of --reps: segment_std from a host array and from a
DeviceMatrix, fitted_curves (noised, left on the device), linkage_of_rows (complete) from the device curves, flat_clusters (host),
curve_activities, and the three chained as tl.genes_selection_analysis runs them (spreads -> curves -> linkage -> activities).
Restatement parts: groupby().std(), make_curves + StandardScaler, pdist, linkage, fcluster, activities; a case with more than
--cpu-max-g genes runs the whole restatement on its first --cpu-max-g genes only and says so.  Also prints the
largest |device - restatement| of the spreads and curves and whether the flat clusters agree.  Writes OUT/gene_curves_rate.txt
(--out, default profiles/gene_curves/)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gene_curves"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="2000x200x50000,20000x600x200000")
    ap.add_argument("--cpu-max-g", type=int, default=6000)
    ap.add_argument("--method", default="complete")
    a = ap.parse_args()
    import curves_restatement as CR
    from pilot_amd import _lib, engine
    if _lib.device_count() < 1:
        raise SystemExit("gene_curves_rate.py needs a HIP device: there is no CPU path to time")
    os.makedirs(a.out, exist_ok=True)
    lines = ["device: %s" % _lib.device_name()]
    for case in a.cases.split(","):
        G, T, n = (int(v) for v in case.split("x"))
        rng = np.random.default_rng(G + T)
        params, names, times = CR.synthetic_table(rng, G, T)
        model = np.array([CR.MODELS.index(m) for m in names], dtype=np.int32)
        t = np.sort(np.r_[np.repeat(np.arange(1, T + 1), 2), rng.integers(1, T + 1, n - 2 * T)]).astype(np.float64)
        offsets = np.r_[np.unique(t, return_index=True)[1], n]
        Y = rng.random((n, G), dtype=np.float32)
        gb = Y.nbytes / 1e9
        s_host, sd = timed(lambda: engine.segment_std(Y, offsets), a.reps)
        dY = engine.DeviceMatrix.upload(Y)
        s_dev, dsd = timed(lambda: engine.segment_std(dY, offsets, device=True), a.reps)
        s_cur, dcur = timed(lambda: engine.fitted_curves(params, model, times, noise=dsd, device=True), a.reps)
        s_link, (Z, dmax, info) = timed(lambda: engine.linkage_of_rows(dcur, a.method, return_info=True), a.reps)
        s_flat, labels = timed(lambda: engine.flat_clusters(Z, 0.4 * dmax), 1)
        s_act, act = timed(lambda: engine.curve_activities(dcur, times), a.reps)

        def chain():
            d1 = engine.segment_std(dY, offsets, device=True)
            d2 = engine.fitted_curves(params, model, times, noise=d1, device=True)
            z, dm = engine.linkage_of_rows(d2, a.method)
            return engine.flat_clusters(z, 0.4 * dm), engine.curve_activities(d2, times)
        s_chain, _ = timed(chain, a.reps)
        lines.append("G=%d T=%d cells=%d (%.2f GB f32) DEVICE: segment_std %.1f ms from HBM (%.0f GB/s of Y), %.1f ms from a host array; "
                     "fitted_curves %.2f ms; linkage_of_rows(%s) %.1f ms (%d chain steps); flat_clusters (host) %.1f ms; "
                     "curve_activities %.2f ms; chained %.1f ms"
                     % (G, T, n, gb, s_dev * 1e3, gb / s_dev, s_host * 1e3, s_cur * 1e3, a.method, s_link * 1e3, info["chain_steps"],
                        s_flat * 1e3, s_act * 1e3, s_chain * 1e3))
        # the restatement on the CPUs of the same box
        Gc = min(G, a.cpu_max_g)                                   # the restatement's share of the genes (all of them if G fits)
        t0 = time.perf_counter(); _, sd_r = CR.segment_std(Y[:, :Gc], t); c_std = time.perf_counter() - t0
        t0 = time.perf_counter(); _, sn = CR.noised_curves(params[:Gc], names[:Gc], times, sd_r); c_cur = time.perf_counter() - t0
        sub = sn
        t0 = time.perf_counter(); d = CR.sch.distance.pdist(sub); c_pd = time.perf_counter() - t0
        t0 = time.perf_counter(); Zr = CR.sch.linkage(d, method=a.method); c_link = time.perf_counter() - t0
        t0 = time.perf_counter(); lab_r = CR.sch.fcluster(Zr, 0.4 * d.max(), "distance"); c_flat = time.perf_counter() - t0
        t0 = time.perf_counter(); CR.activities_raw(sn, times); c_act = time.perf_counter() - t0
        cur = engine.download(dcur)
        agree = "flat clusters equal: %s" % np.array_equal(labels, lab_r) if Gc == G else \
            "the restatement ran on the first %d genes only (its clusters are not compared)" % Gc
        lines.append("G=%d T=%d cells=%d RESTATEMENT: groupby.std %.2f s; curves + StandardScaler %.2f s; pdist %.2f s; linkage %.2f s; "
                     "fcluster %.3f s; activities %.3f s; sum %.2f s.  max |device - restatement|: spreads %.2e, curves %.2e; %s"
                     % (G, T, n, c_std, c_cur, c_pd, c_link, c_flat, c_act, c_std + c_cur + c_pd + c_link + c_flat + c_act,
                        np.nanmax(np.abs(sd[:, :Gc] - sd_r)), np.abs(cur[:Gc] - sn).max(), agree))
        for ln in lines[-2:]:
            print(ln, flush=True)
        del Y, dY, dsd, dcur
    with open(os.path.join(a.out, "gene_curves_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
