// The host side of the symmetric Lanczos run that the diffusion map (pilot_ot_diffmap.hip) and the principal components
// (pilot_ot_pca.hip) share: its constants, the launches of one step after the caller's product w = A v_j (kernels:
// lanczos_kernels.hpp), and the implicit-QL solver of the small tridiagonal Ritz problem.  Host-side only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <numeric>
#include <vector>

#include "lanczos_kernels.hpp"

namespace pilot {

constexpr int LZ_MAX_BASIS = 1024;           // B = min(N, LZ_MAX_BASIS) Lanczos vectors (V: B x N f64)
constexpr int LZ_MAX_EVECS = 64;
constexpr int LZ_CHECK_EVERY = 8;            // Lanczos steps between two looks at the tridiagonal problem
// both relative to the operator's norm (the diffusion map's |S| is 1; the principal components scale them)
constexpr double LZ_RESID_TOL = 1e-12;       // |beta_j s_ji| of every wanted Ritz pair
constexpr double LZ_BREAKDOWN_TOL = 1e-12;   // |w| after re-orthogonalisation below which the Krylov space counts as invariant

// Step j after the product: w = A V[j] is orthogonalised against V[0..j] twice, alpha[j] and beta[j] are set and V[j + 1] written
// (lz_finish_kernel; tol: the |w| that counts as a breakdown).  The caller checks hipGetLastError.
inline void lanczos_step(double *V, int N, int j, int B, double *w, double *h1, double *h2, double tol, double *al, double *be,
                         int *n_restart, hipStream_t s) {
    const int nk = j + 1;
    hipLaunchKernelGGL(lz_dots_kernel, dim3(nk), dim3(DM_RED), 0, s, V, N, w, h1);
    hipLaunchKernelGGL(lz_update_kernel, dim3((N + 63) / 64), dim3(64 * LZ_UPD_WAVES), 0, s, V, N, nk, h1, w);
    hipLaunchKernelGGL(lz_dots_kernel, dim3(nk), dim3(DM_RED), 0, s, V, N, w, h2);
    hipLaunchKernelGGL(lz_update_kernel, dim3((N + 63) / 64), dim3(64 * LZ_UPD_WAVES), 0, s, V, N, nk, h2, w);
    hipLaunchKernelGGL(lz_finish_kernel, dim3(1), dim3(DM_FIN), 0, s, V, N, j, B, w, h1, h2, tol, al, be, n_restart);
}

// Implicit QL with Wilkinson shifts on the symmetric tridiagonal matrix with diagonal d[0..n) and off-diagonal e[0..n-1)
// (e[i] couples i and i + 1; e must have n entries, e[n-1] is scratch).  Eigenvalues overwrite d (unsorted); every rotation is
// applied to the nrows rows of z (row-major nrows x n): start from the identity for the eigenvectors as columns, or from the
// last unit row alone for just their last components.  false if an eigenvalue needed more than 60 iterations.
inline bool tridiag_ql(int n, double *d, double *e, double *z, int nrows) {
    e[n - 1] = 0.0;
    for (int l = 0; l < n; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < n - 1; ++m)
                if (std::fabs(e[m]) <= DBL_EPSILON * (std::fabs(d[m]) + std::fabs(d[m + 1]))) break;
            if (m == l) break;
            if (++iter > 60) return false;
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = std::hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));          // the shift: the eigenvalue of the leading 2 x 2 nearer d[l]
            double s = 1.0, c = 1.0, p = 0.0;
            int i;
            for (i = m - 1; i >= l; --i) {
                double f = s * e[i];
                const double b = c * e[i];
                r = std::hypot(f, g);
                e[i + 1] = r;
                if (r == 0.0) { d[i + 1] -= p; e[m] = 0.0; break; }   // (underflow: the block splits, sweep again)
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                for (int k = 0; k < nrows; ++k) {
                    double *zk = z + (size_t)k * n;
                    f = zk[i + 1];
                    zk[i + 1] = s * zk[i] + c * f;
                    zk[i] = c * zk[i] - s * f;
                }
            }
            if (r == 0.0 && i >= l) continue;
            d[l] -= p;
            e[l] = g;
            e[m] = 0.0;
        } while (true);
    }
    return true;
}

// indices of d sorted by value, largest first (ties: lower index first)
inline std::vector<int> order_desc(const std::vector<double> &d) {
    std::vector<int> ix(d.size());
    std::iota(ix.begin(), ix.end(), 0);
    std::stable_sort(ix.begin(), ix.end(), [&](int a, int b) { return d[a] > d[b]; });
    return ix;
}

}  // namespace pilot
