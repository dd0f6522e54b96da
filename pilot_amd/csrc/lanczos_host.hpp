// The host side of the symmetric Lanczos run that the diffusion map (pilot_ot_diffmap.hip) and the principal components
// (pilot_ot_pca.hip) share: its constants, the launches of one step after the caller's product w = A v_j (kernels:
// lanczos_kernels.hpp), and the implicit-QL solver of the small tridiagonal Ritz problem.  Host-side only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
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

// One run: what is asked for ...
struct LanczosSpec {
    int N;                       // order of the operator
    int B;                       // basis vectors, want <= B <= LZ_MAX_BASIS (below N no complete basis can be reached)
    int want;                    // wanted leading Ritz pairs
    double breakdown;            // the |w| that counts as a breakdown
    double norm;                 // the operator's norm, the scale of LZ_RESID_TOL; 0: the leading Ritz value
    double floor_rel;            // eigenvalues <= floor_rel * (leading Ritz value) count as zero; 0: none do
    bool start_is_eigenvector;   // V[0] is a known eigenvector: step 0 breaks down by construction and the search starts at V[1]
};
// ... and what came of it: the Ritz pairs of the result are those of T = (ha, hb) on V[0 .. nk)
struct LanczosRun {
    std::vector<double> ha, hb;
    int nk = 0;
    int steps = 0;               // Lanczos steps the basis held when the run stopped, the verification block included
    bool converged = false;
};

// Single-vector Lanczos with full re-orthogonalisation and the acceptance rule.  product(v, w) launches w = A v on s.
//
// A Krylov space grown from one vector holds one direction per distinct eigenvalue, so converged Ritz pairs alone do not show that
// the wanted part of the spectrum is complete: a second copy of a wanted eigenvalue is invisible to it.  A result is accepted only
//   (a) from a complete basis (N steps: T is similar to A), or
//   (b) when, after the wanted pairs converged (|beta_j s_ji| <= LZ_RESID_TOL * norm) or the Krylov space broke down, a verification
//       block -- Lanczos from the next restart vector, orthogonalised against the whole basis so far, so Lanczos on A compressed to
//       the complement -- has a largest Ritz value that itself converged (or whose Krylov space broke down or filled the
//       complement) and lies below the smallest wanted Ritz value by more than the residual tolerance, or at or below the floor.
//       The result is then the Ritz pairs of the basis as it stood when the block began.
// A verification block that finds something at or above the smallest wanted value (or fewer than `want` pairs before a breakdown
// with a non-zero complement) is followed by a complete basis when B = N: the steps of the block are dropped, the step before it is
// taken again as a plain Lanczos step unless it was a breakdown, and the run goes on to N steps.  With B < N, or without room
// for a block, the run is not converged.  With start_is_eigenvector, a breakdown after step 0 accepts only a complete basis.
template <class Product>
inline hipError_t lanczos_run(const LanczosSpec &sp, double *V, double *w, double *h1, double *h2, double *al, double *be, int *n_restart,
                              hipStream_t s, Product &&product, LanczosRun *run) {
    const int N = sp.N, B = sp.B, m = sp.want;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> ha(B), hb(B), d, e, z;
    std::vector<int> ix;
    auto ritz = [&](int a, int b) {                           // Ritz values of T[a, b) and the last components of their vectors
        d.assign(ha.begin() + a, ha.begin() + b);
        e.assign(hb.begin() + a, hb.begin() + b);
        z.assign(b - a, 0.0);
        z[b - a - 1] = 1.0;
        return tridiag_ql(b - a, d.data(), e.data(), z.data(), 1);
    };
    enum { SEARCH, VERIFY, COMPLETE } mode = SEARCH;
    int steps = 0, next_check = m, acc = 0;                    // acc: the basis at first acceptance (0: none, the whole basis counts)
    bool forced = false, converged = false;
    double tol = 0.0, smallest = -inf, floor = -inf;
    while (steps < B) {
        const int j = steps;
        product(V + (size_t)j * N, w);
        lanczos_step(V, N, j, B, w, h1, h2, sp.breakdown, al, be, n_restart, s);
        if (hipError_t err = hipGetLastError()) return err;
        steps = j + 1;
        if (steps < next_check && steps < B) continue;
        next_check = steps + LZ_CHECK_EVERY;
        if (hipError_t err = hipMemcpyAsync(ha.data(), al, sizeof(double) * steps, hipMemcpyDeviceToHost, s)) return err;
        if (hipError_t err = hipMemcpyAsync(hb.data(), be, sizeof(double) * steps, hipMemcpyDeviceToHost, s)) return err;
        if (hipError_t err = hipStreamSynchronize(s)) return err;
        if (mode == SEARCH) {
            // a breakdown: the Krylov space of the start vector is invariant and its Ritz pairs are eigenpairs, one per distinct
            // eigenvalue that the start vector has a component of; what lies outside it is for the verification block
            int first = -1;
            for (int q = 0; q < steps && first < 0 && !sp.start_is_eigenvector; ++q)
                if (hb[q] == 0.0) first = q;
            if (first >= 0) {
                acc = first + 1;
                if (!ritz(0, acc)) { acc = 0; break; }    // (the caller's own QL of T fails the same way and reports it)
                ix = order_desc(d);
            } else {
                if (steps == N) { converged = true; break; }   // a complete basis: T is similar to A
                // a breakdown after that of step 0 means the Krylov space of a restart vector was exhausted; what lies outside
                // it is unexplored, so only a complete basis is accepted from then on
                bool late_breakdown = false;
                for (int k = 1; k < steps; ++k) late_breakdown |= hb[k] == 0.0;
                if (late_breakdown) { mode = COMPLETE; next_check = N; continue; }
                if (!ritz(0, steps)) continue;
                ix = order_desc(d);
                const double t = LZ_RESID_TOL * (sp.norm > 0.0 ? sp.norm : d[ix[0]]);
                bool ok = true;
                for (int c = 0; c < m; ++c) ok &= std::fabs(hb[steps - 1] * z[ix[c]]) <= t;
                if (!ok) continue;
                acc = steps;
                forced = true;
            }
            run->ha.assign(ha.begin(), ha.begin() + acc);
            run->hb.assign(hb.begin(), hb.begin() + acc);
            if (acc == N) { converged = true; break; }         // (the breakdown of the last step of a complete basis)
            if (acc >= B) break;                               // no room to look behind the result
            const double lam0 = d[ix[0]];
            tol = LZ_RESID_TOL * (sp.norm > 0.0 ? sp.norm : lam0);
            smallest = acc >= m ? d[ix[m - 1]] : -inf;
            floor = sp.floor_rel > 0.0 ? sp.floor_rel * lam0 : -inf;
            mode = VERIFY;
            if (forced) {
                hipLaunchKernelGGL(lz_restart_kernel, dim3(1), dim3(DM_FIN), 0, s, V, N, acc - 1, w, be, n_restart);
                if (hipError_t err = hipGetLastError()) return err;
            }
            if (steps == acc) { next_check = steps + 1; continue; }
        }
        if (mode == VERIFY) {
            int end = steps;                                   // the block: T[acc, end), up to its own first breakdown
            for (int q = steps - 1; q >= acc; --q)
                if (hb[q] == 0.0) end = q + 1;
            if (!ritz(acc, end)) continue;
            const int top = (int)(std::max_element(d.begin(), d.end()) - d.begin());
            const bool closed = hb[end - 1] == 0.0 || end == N;
            if (!closed && std::fabs(hb[end - 1] * z[top]) > tol) continue;
            if (d[top] < smallest - tol || d[top] <= floor) { converged = true; break; }
            if (B < N) break;                                  // something is hidden and no complete basis can show it
            mode = COMPLETE;
            next_check = N;
            if (forced) steps = acc - 1;                       // step acc - 1 again: its own next vector, not the restart vector
            acc = 0;
        }
        if (mode == COMPLETE && steps == N) { converged = true; break; }
    }
    if (acc == 0) {
        run->ha.assign(ha.begin(), ha.begin() + steps);
        run->hb.assign(hb.begin(), hb.begin() + steps);
    }
    run->nk = acc ? acc : steps;
    run->steps = steps;
    run->converged = converged;
    return hipSuccess;
}

}  // namespace pilot
