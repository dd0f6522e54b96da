#!/usr/bin/env python3
"""Pin the diffusion-map restatement (tests/diffmap_restatement.py) to the real pydiffmap, wherever pydiffmap installs (CPU only).

The restatement of pydiffmap 0.2.x -- the 'or' symmetrisation, the 4 epsilon of the kernel, the sqrt(-1 / lambda) scaling -- was
written from memory (unpinned).  This runs pl.trajectory's own call (pilotpy/plot/ploting.py:109-110)
    DiffusionMap.from_sklearn(n_evecs, epsilon, alpha, k).fit_transform(EMD / EMD.max())
on the stored matrices of the golden fixtures and compares it with the restatement, column by column up to sign.  Prints PINNED,
or the first disagreements; without pydiffmap it says so and exits 0."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diffmap_restatement as R  # noqa: E402

CASES = [("c1_20x10x10", 5, 1.0, 0.5, 2), ("c1_20x10x10", 16, 0.3, 0.0, 5), ("c2s_100x30x30", 64, 1.0, 0.5, 2),
         ("c2s_100x30x30", 16, 0.3, 1.0, 5), ("kidney_igan_g_634x14x14", 64, 1.0, 0.5, 2)]
TOL = 1e-6


def main():
    try:
        from pydiffmap import diffusion_map
    except Exception as e:                                        # noqa: BLE001 -- any import failure means "not here"
        print("pydiffmap not importable (%s: %s): nothing pinned" % (type(e).__name__, e))
        return 0
    bad = []
    for name, k, eps, alpha, n_evecs in CASES:
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False)
        E = z["emd_unreg"]
        if E.shape[0] != E.shape[1]:                            # (fixtures that store a row subset of the matrix)
            print("%-26s skipped: the fixture stores %d of its rows" % (name, E.shape[0]))
            continue
        X = E / E.max()
        got = diffusion_map.DiffusionMap.from_sklearn(n_evecs=n_evecs, epsilon=eps, alpha=alpha, k=k).fit_transform(X)
        want, _, _ = R.diffusion_map_of_rows(E, n_evecs=n_evecs, epsilon=eps, alpha=alpha, k=k)
        want = R.align_signs(got, want)
        err = np.abs(got - want).max(0) / np.abs(want).max(0)
        status = "ok" if err.max() <= TOL else "DIFFERS"
        print("%-26s k=%-3d eps=%-4g alpha=%-4g n_evecs=%d  max rel |pydiffmap - restatement| per column %s  %s"
              % (name, k, eps, alpha, n_evecs, np.array2string(err, precision=2), status))
        if status != "ok":
            bad.append(name)
    print("PINNED" if not bad else "NOT PINNED: %s" % bad)
    return 0 if not bad else 1


if __name__ == "__main__":
    sys.exit(main())
