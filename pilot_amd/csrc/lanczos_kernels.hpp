// Symmetric Lanczos with full re-orthogonalisation, the part that does not care what the operator is: given w = A v_j, a step
// takes the two classical Gram-Schmidt passes against the basis, alpha_j, beta_j and the next basis vector (or, on a breakdown, the
// documented restart vector); the Ritz kernel turns the eigenvectors of the tridiagonal matrix into vectors of the problem.  K8 (the
// diffusion map, diffmap_kernels.hpp) and K15 (principal components, pca_kernels.hpp) bring their own product; the host side of a
// step is lanczos_host.hpp.
//
// Everything is f64.  Every sum is taken in a fixed order (per-thread strided partial sums, then a fixed LDS / shuffle tree), and
// nothing uses floating-point atomics: a call repeated on the same input gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "reduce.hpp"

namespace pilot {

constexpr int DM_RED = 256;            // threads of the row-reduction / dot-product workgroups
constexpr int DM_FIN = 1024;           // threads of the single-workgroup step finish

// h[k] = V[k] . w for k < nk: one workgroup (DM_RED threads) per basis vector
static __global__ void __launch_bounds__(DM_RED) lz_dots_kernel(const double *__restrict__ V, int N, const double *__restrict__ w,
                                                                double *__restrict__ h) {
    __shared__ double red[DM_RED];
    const double *vk = V + (size_t)blockIdx.x * N;
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += DM_RED) s += vk[n] * w[n];
    s = block_tree_sum<DM_RED>(s, red);
    if (threadIdx.x == 0) h[blockIdx.x] = s;
}

// w -= sum_k h[k] V[k] (k < nk).  A workgroup owns 64 consecutive entries; its 16 waves take the basis vectors k = wave, wave + 16,
// ... (coalesced 64-entry reads of a basis vector), and the 16 partial sums are added in wave order.
constexpr int LZ_UPD_WAVES = 16;
static __global__ void __launch_bounds__(64 * LZ_UPD_WAVES) lz_update_kernel(const double *__restrict__ V, int N, int nk,
                                                                             const double *__restrict__ h, double *__restrict__ w) {
    __shared__ double part[LZ_UPD_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (n < N)
        for (int k = wv; k < nk; k += LZ_UPD_WAVES) s += h[k] * V[(size_t)k * N + n];
    part[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && n < N) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < LZ_UPD_WAVES; ++q) t += part[q][lane];
        w[n] -= t;
    }
}

// The documented restart vector (Lanczos breakdown): entry n of restart number c is a splitmix64 hash of (n, c) mapped to
// [-1, 1) -- r_n = 2 * (z >> 11) * 2^-53 - 1 with z = splitmix64((c + 1) * 2^32 + n).
__device__ inline double lz_restart_entry(int n, int c) {
    unsigned long long z = ((unsigned long long)(c + 1) << 32) + (unsigned long long)n;
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return 2.0 * ((double)(z >> 11) * 0x1.0p-53) - 1.0;
}

// V[j + 1] = the next restart vector (number *n_restart, which is counted up), orthogonalised against V[0..j] by two classical
// Gram-Schmidt passes and normalised.  For every thread of a workgroup of DM_FIN threads; w (N) is overwritten, red (DM_FIN) and
// hs (1024 >= j + 1) are LDS.
__device__ inline void lz_restart_into(double *__restrict__ V, int N, int j, double *__restrict__ w, int *__restrict__ n_restart,
                                       double *red, double *hs) {
    const int c = *n_restart;
    __syncthreads();
    if (threadIdx.x == 0) *n_restart = c + 1;
    for (int n = threadIdx.x; n < N; n += DM_FIN) w[n] = lz_restart_entry(n, c);
    __syncthreads();
    const int nk = j + 1, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = wv; k < nk; k += DM_FIN / 64) {           // one wave per dot product
            const double *vk = V + (size_t)k * N;
            double t = 0.0;
            for (int n = lane; n < N; n += 64) t += vk[n] * w[n];
            t = lanes_sum(t);
            if (lane == 0) hs[k] = t;
        }
        __syncthreads();
        for (int n = threadIdx.x; n < N; n += DM_FIN) {
            double t = 0.0;
            for (int k = 0; k < nk; ++k) t += hs[k] * V[(size_t)k * N + n];
            w[n] -= t;
        }
        __syncthreads();
    }
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += DM_FIN) s += w[n] * w[n];
    const double r = sqrt(block_tree_sum<DM_FIN>(s, red));
    for (int n = threadIdx.x; n < N; n += DM_FIN) V[(size_t)(j + 1) * N + n] = w[n] / r;
}

// End of Lanczos step j (basis V[0..j] holds j + 1 vectors, w = S v_j after the two Gram-Schmidt passes with coefficients h1, h2):
//   alpha[j] = h1[j] + h2[j];  beta[j] = |w|;  V[j + 1] = w / beta[j]  (when j + 1 < B).
// Breakdown (beta[j] <= tol: the Krylov space is invariant -- at step 0 always, since V[0] is an eigenvector): beta[j] = 0 and
// V[j + 1] is the next restart vector (lz_restart_into); the restart count lives in *n_restart.  One workgroup of DM_FIN threads;
// w is overwritten.
static __global__ void __launch_bounds__(DM_FIN) lz_finish_kernel(double *__restrict__ V, int N, int j, int B, double *__restrict__ w,
                                                                  const double *__restrict__ h1, const double *__restrict__ h2,
                                                                  double tol, double *__restrict__ alpha, double *__restrict__ beta,
                                                                  int *__restrict__ n_restart) {
    __shared__ double red[DM_FIN];
    __shared__ double hs[1024];                               // (B <= 1024)
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += DM_FIN) s += w[n] * w[n];
    const double b = sqrt(block_tree_sum<DM_FIN>(s, red));
    if (threadIdx.x == 0) alpha[j] = h1[j] + h2[j];
    if (b > tol) {
        if (threadIdx.x == 0) beta[j] = b;
        if (j + 1 < B)
            for (int n = threadIdx.x; n < N; n += DM_FIN) V[(size_t)(j + 1) * N + n] = w[n] / b;
        return;
    }
    if (threadIdx.x == 0) beta[j] = 0.0;
    if (j + 1 >= B) return;                                   // (basis complete: nothing to continue with)
    lz_restart_into(V, N, j, w, n_restart, red, hs);
}

// The start of a verification block after step j (j + 1 < B <= 1024), without a breakdown: beta[j] = 0 and V[j + 1] is the next
// restart vector in place of the Krylov vector that step j wrote there.  One workgroup of DM_FIN threads; w is overwritten.
static __global__ void __launch_bounds__(DM_FIN) lz_restart_kernel(double *__restrict__ V, int N, int j, double *__restrict__ w,
                                                                   double *__restrict__ beta, int *__restrict__ n_restart) {
    __shared__ double red[DM_FIN];
    __shared__ double hs[1024];
    if (threadIdx.x == 0) beta[j] = 0.0;
    lz_restart_into(V, N, j, w, n_restart, red, hs);
}

// Ritz vectors and the back-transform: psi[n][c] = dis[n] * sum_k Z[k][c] V[k][n] (k < nk, in order), c < m.  Z: nk x m row-major.
// psi: N x m row-major.  One thread per (n, c).  dis == nullptr: no back-transform, the sum as it is.
static __global__ void lz_ritz_kernel(const double *__restrict__ V, int N, int nk, const double *__restrict__ Z, int m,
                                      const double *__restrict__ dis, double *__restrict__ psi) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)N * m) return;
    const int n = (int)(t / m), c = (int)(t % m);
    double s = 0.0;
    for (int k = 0; k < nk; ++k) s += Z[(size_t)k * m + c] * V[(size_t)k * N + n];
    psi[t] = dis ? s * dis[n] : s;
}

}  // namespace pilot
