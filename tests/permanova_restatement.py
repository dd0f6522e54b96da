"""K29 (PERMANOVA) restated in numpy by another route than the kernels': Philox4x32-10 in uint64 arithmetic, the order by
``np.lexsort``, the sums of squares as ``np.longdouble`` sums of ``z_i A_ij z_j`` with the magnitude sums the error bounds need.
No device, no library call."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
EPS = float(np.sqrt(2.0 ** -52))


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> the four output words, uint64 arrays holding 32 bits"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]              # 32 x 32 bits: no overflow in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def row_keys(n, b, seed):
    """k_i = w0 2^32 + w1 of rows 0 .. n-1 in permutation b"""
    i = np.arange(n, dtype=np.uint64)
    w = philox4x32_10((i, b & 0xFFFFFFFF, b >> 32, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return (w[0] << np.uint64(32)) | w[1]


def strata_codes(n, strata):
    if strata is None:
        return np.zeros(n, dtype=np.int64)
    codes = np.unique(np.asarray(strata), return_inverse=True)[1].astype(np.int64)
    assert codes.shape == (n,)
    return codes


def permutation(n, b, seed, strata=None):
    """p with Z_b[i, :] = Q[p[i], :]: p[r_t] = s_t, s the rows by (stratum, key, i), r the rows by (stratum, i)"""
    idx = np.arange(n)
    if b == 0:
        return idx
    st = strata_codes(n, strata)
    s = np.lexsort((idx, row_keys(n, b, seed), st))
    r = np.lexsort((idx, st))
    p = np.empty(n, dtype=np.int64)
    p[r] = s
    return p


def permutations(n, n_perm, seed, strata=None, start=0):
    return np.stack([permutation(n, b, seed, strata) for b in range(start, n_perm + 1)]).astype(np.int32)


def a_matrix(D, rows=None):
    """s_ij = (D_ij + D_ji) / 2, s_ii = 0, A_ij = -0.5 s_ij s_ij of the used rows, in float64, these operations in this order"""
    D = np.asarray(D).astype(np.float64)
    if rows is not None:
        D = D[np.ix_(rows, rows)]
    S = (D + D.T) / 2
    np.fill_diagonal(S, 0.0)
    return -0.5 * S * S


def ss_total(A):
    """(-(1/n) sum A_ij, (1/n) sum |A_ij|) in long double"""
    L = A.astype(np.longdouble)
    n = np.longdouble(A.shape[0])
    return -(L.sum() / n), np.abs(L).sum() / n


def column_form(A, z):
    """(z^T A z, sum_ij |z_i| |A_ij| |z_j|) in long double"""
    L, z = A.astype(np.longdouble), z.astype(np.longdouble)
    return (z[:, None] * L * z[None, :]).sum(), (np.abs(z)[:, None] * np.abs(L) * np.abs(z)[None, :]).sum()


def ss_terms(A, Q, terms, perms):
    """(ss, mag): len(perms) x terms long-double arrays, ss[b, t] = sum over the term's columns of Z_b[:, c]^T A Z_b[:, c] and the
    sum of magnitudes beside it"""
    n_terms = len(terms) - 1
    ss = np.zeros((len(perms), n_terms), dtype=np.longdouble)
    mag = np.zeros_like(ss)
    for b, p in enumerate(perms):
        Z = Q[p]
        for t in range(n_terms):
            for c in range(terms[t], terms[t + 1]):
                v, m = column_form(A, Z[:, c])
                ss[b, t] += v
                mag[b, t] += m
    return ss, mag


def f_stat(total, ss, terms, n):
    q = np.diff(np.asarray(terms)).astype(np.longdouble)
    return (ss / q) / ((total - ss) / (np.longdouble(n) - q - 1))


def p_values(F):
    return (1.0 + np.count_nonzero(F[1:] >= F[0] - np.longdouble(EPS), axis=0)) / float(F.shape[0])
