"""The point clouds of the principal-tree tests (test_principal_tree_args.py, test_gpu_principal_tree.py): a noisy half circle
("arc"), three noisy branches from the origin in the plane ("y") and in five dimensions ("y5")."""
import numpy as np

# whole trees (name, n, M, seed) and single fits (name, n, m, seed): inputs whose every discrete decision is far from its edge
TREES = [("arc", 120, 8, 1), ("y", 300, 12, 2), ("y5", 600, 20, 3), ("arc", 40, 6, 4), ("y", 150, 10, 7), ("y5", 257, 9, 5)]
FITS = [("arc", 40, 3, 4), ("arc", 65, 5, 11), ("y5", 100, 6, 12), ("y", 257, 7, 13)]


def cloud(name, n, seed):
    r = np.random.default_rng(seed)
    if name == "arc":
        t = r.uniform(0, np.pi, n); return np.c_[np.cos(t), np.sin(t)] + 0.05 * r.normal(size=(n, 2))
    t = r.uniform(0, 1, n); br = r.integers(0, 3, n)
    if name == "y":
        return t[:, None] * np.array([[0, -1.0], [0.8, 0.7], [-0.9, 0.5]])[br] + 0.04 * r.normal(size=(n, 2))
    dirs = r.normal(size=(3, 5)); return t[:, None] * dirs[br] + 0.05 * r.normal(size=(n, 5))      # "y5"


def path_springs(m, lam=0.01, mu=0.1):
    """the spring matrix of the path 0 - 1 - ... - (m - 1), by the definition"""
    S = np.zeros((m, m))
    for a in range(m - 1):
        v = np.zeros(m); v[a], v[a + 1] = 1.0, -1.0
        S += lam * np.outer(v, v)
    for c in range(1, m - 1):
        s = np.zeros(m); s[c], s[c - 1], s[c + 1] = 1.0, -0.5, -0.5
        S += mu * np.outer(s, s)
    return S


def fit_case(name, n, m, seed, dtype):
    """(X of `dtype`, Y0 = m of its points, path springs, centre) of a single fit"""
    X = np.ascontiguousarray(cloud(name, n, seed).astype(dtype))
    Y0 = X[np.random.default_rng(seed).choice(n, m, replace=False)].astype(np.float64)
    return X, Y0, path_springs(m), X.astype(np.float64).mean(axis=0)
