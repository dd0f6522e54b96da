// K16, the graph half: the per-row part of UMAP's fuzzy simplicial set over the distances knn_rows_kernel (knn_kernels.hpp) returns.
// Included by pilot_ot_knn.hip alone: the kernel is not a template, so it lives in one translation unit.
#pragma once
#include <hip/hip_runtime.h>

namespace pilot {

// ---- the per-row part of UMAP's fuzzy simplicial set (tests/neighbors_restatement.py states the same rule) ---------------------
constexpr int KNN_SMOOTH_STEPS = 64;
constexpr double KNN_SMOOTH_TOL = 1e-5;
constexpr double KNN_SMOOTH_FLOOR = 1e-3;

// dist: n x k distances to the k = n_neighbors - 1 other cells, ascending.  rho = the smallest non-zero one (0: none).  sigma: the
// bisection of sum_j exp(-max(0, d_j - rho) / sigma) = log2(k + 1), floored at KNN_SMOOTH_FLOOR x the row's mean distance (rho > 0)
// or x global_mean (rho = 0).  weights = 1 where d_j - rho <= 0 or sigma = 0, else exp(-(d_j - rho) / sigma).  One row per thread.
__global__ void knn_smooth_kernel(const double *__restrict__ dist, long long n, int k, double global_mean, double *__restrict__ weights,
                                  double *__restrict__ sigma, double *__restrict__ rho) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *d = dist + i * k;
    const double target = log2((double)(k + 1));
    double r = 0.0, mean = 0.0;
    for (int c = 0; c < k; ++c) {
        mean += d[c];
        if (d[c] > 0.0 && (r == 0.0 || d[c] < r)) r = d[c];
    }
    mean /= (double)k;
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int it = 0; it < KNN_SMOOTH_STEPS; ++it) {
        double psum = 0.0;
        for (int c = 0; c < k; ++c) {
            const double g = d[c] - r;
            psum += g > 0.0 ? exp(-(g / mid)) : 1.0;
        }
        if (fabs(psum - target) < KNN_SMOOTH_TOL) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = isinf(hi) ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    const double floor = KNN_SMOOTH_FLOOR * (r > 0.0 ? mean : global_mean);
    if (mid < floor) mid = floor;
    for (int c = 0; c < k; ++c) {
        const double g = d[c] - r;
        weights[i * k + c] = (g <= 0.0 || mid == 0.0) ? 1.0 : exp(-(g / mid));
    }
    sigma[i] = mid;
    rho[i] = r;
}

}  // namespace pilot
