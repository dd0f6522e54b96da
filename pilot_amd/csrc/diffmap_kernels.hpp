// K8: the eigen-part of pl.trajectory's diffusion map (pilotpy/plot/ploting.py:109-110, pydiffmap's DiffusionMap with a numeric
// epsilon, no weight function, no bandwidth normalisation) on the k-nearest-neighbour kernel K7 leaves in HBM.
//
//   Ks = max(K, K^T)                      (pydiffmap's 'or' symmetrisation)
//   q  = Ks.sum(1),  qa = q^-alpha        (right normalisation Ks diag(qa))
//   d  = qa * (Ks qa)                     (row sums of A = diag(qa) Ks diag(qa))
//   S  = D^-1/2 A D^-1/2 = Ks_ij * (w_i w_j),  w = qa / sqrt(d)
// S is symmetric and similar to pydiffmap's Markov matrix P = D^-1 A: S phi = mu phi  <=>  P (D^-1/2 phi) = mu (D^-1/2 phi).  Its
// top eigenpairs come from a symmetric Lanczos run with full re-orthogonalisation (two classical Gram-Schmidt passes a step); the
// host solves the small tridiagonal problem (pilot_ot_diffmap.hip).
//
// Everything is f64.  Every sum is taken in a fixed order (per-thread strided partial sums, then a fixed LDS / shuffle tree), and
// nothing uses floating-point atomics: a call repeated on the same input gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "lanczos_kernels.hpp"
#include "reduce.hpp"

namespace pilot {

constexpr int DM_TILE = 32;            // transpose tile of the symmetrisation

// Ks[i][j] = max(K[i][j], K[j][i]); 32 x 32 tiles through LDS so both the row and the transposed read are coalesced.
// grid (ceil(N/32), ceil(N/32)), block (32, 8).  Ks must not alias K.
static __global__ void __launch_bounds__(256) dm_symmetrize_kernel(const double *__restrict__ K, int N, double *__restrict__ Ks) {
    __shared__ double t[DM_TILE][DM_TILE + 1];
    const int bi = blockIdx.y * DM_TILE, bj = blockIdx.x * DM_TILE;
    // stage the transposed tile: rows bj.., columns bi.. of K
    for (int r = threadIdx.y; r < DM_TILE; r += blockDim.y) {
        const int gi = bj + r, gj = bi + (int)threadIdx.x;
        t[r][threadIdx.x] = (gi < N && gj < N) ? K[(size_t)gi * N + gj] : 0.0;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < DM_TILE; r += blockDim.y) {
        const int gi = bi + r, gj = bj + (int)threadIdx.x;
        if (gi < N && gj < N) {
            const double a = K[(size_t)gi * N + gj], b = t[threadIdx.x][r];      // K[gi][gj], K[gj][gi]
            Ks[(size_t)gi * N + gj] = a > b ? a : b;
        }
    }
}

// One workgroup (DM_RED threads) per row i of the symmetrised kernel.
// mode 0:  qa[i] = (sum_j Ks[i][j])^-alpha
// mode 1:  r = sum_j Ks[i][j] qa[j];  d = qa[i] r;  w[i] = qa[i] / sqrt(d);  dis[i] = 1 / sqrt(d);  phi[i] = sqrt(d)
static __global__ void __launch_bounds__(DM_RED) dm_row_kernel(const double *__restrict__ Ks, int N, int mode, double alpha,
                                                               double *__restrict__ qa, double *__restrict__ w,
                                                               double *__restrict__ dis, double *__restrict__ phi) {
    __shared__ double red[DM_RED];
    const int i = blockIdx.x;
    const double *row = Ks + (size_t)i * N;
    double s = 0.0;
    if (mode == 0) for (int j = threadIdx.x; j < N; j += DM_RED) s += row[j];
    else           for (int j = threadIdx.x; j < N; j += DM_RED) s += row[j] * qa[j];
    s = block_tree_sum<DM_RED>(s, red);
    if (threadIdx.x == 0) {
        if (mode == 0) qa[i] = pow(s, -alpha);
        else {
            const double d = qa[i] * s, sd = sqrt(d);
            w[i] = qa[i] / sd;
            dis[i] = 1.0 / sd;
            phi[i] = sd;
        }
    }
}

// S[i][j] = Ks[i][j] * (w[i] * w[j]) in place (the product of the two scales first: S is symmetric bit for bit)
static __global__ void dm_scale_kernel(double *__restrict__ S, int N, const double *__restrict__ w) {
    const size_t n = (size_t)N * N;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(t / N), j = (int)(t % N);
        S[t] *= w[i] * w[j];
    }
}

// V[0] = phi / |phi|: the known top eigenvector of S (mu = 1), sqrt(d).  One workgroup of DM_FIN threads.
static __global__ void __launch_bounds__(DM_FIN) lz_start_kernel(const double *__restrict__ phi, int N, double *__restrict__ V) {
    __shared__ double red[DM_FIN];
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += DM_FIN) s += phi[n] * phi[n];
    const double nrm = sqrt(block_tree_sum<DM_FIN>(s, red));
    for (int n = threadIdx.x; n < N; n += DM_FIN) V[n] = phi[n] / nrm;
}

// w = S v: one wave per row (4 rows per 256-thread workgroup), lanes stride the row, a butterfly adds the 64 partials
static __global__ void __launch_bounds__(256) lz_gemv_kernel(const double *__restrict__ S, int N, const double *__restrict__ v,
                                                             double *__restrict__ w) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= N) return;                                       // (whole waves leave together)
    const double *row = S + (size_t)i * N;
    double s = 0.0;
    for (int j = lane; j < N; j += 64) s += row[j] * v[j];
    s = lanes_sum(s);
    if (lane == 0) w[i] = s;
}

// Column c of psi (N x m row-major): unit 2-norm, sign such that the entry of largest magnitude (lowest index on ties) is
// positive; dmap[n][c] = psi[n][c] * sqrt(-1 / lambda[c]).  One workgroup (DM_RED threads) per column.  evecs (nullable) gets psi.
static __global__ void __launch_bounds__(DM_RED) dm_finalize_kernel(const double *__restrict__ psi, int N, int m,
                                                                    const double *__restrict__ lambda, double *__restrict__ dmap,
                                                                    double *__restrict__ evecs) {
    __shared__ double red[DM_RED];
    __shared__ double bv[DM_RED];
    __shared__ int bi[DM_RED];
    const int c = blockIdx.x;
    double s = 0.0, best = -1.0;
    int at = N;
    for (int n = threadIdx.x; n < N; n += DM_RED) {
        const double x = psi[(size_t)n * m + c];
        s += x * x;
        const double a = fabs(x);
        if (a > best) { best = a; at = n; }                    // (n ascending: the first of equal magnitudes stays)
    }
    const double nrm = sqrt(block_tree_sum<DM_RED>(s, red));
    bv[threadIdx.x] = best; bi[threadIdx.x] = at;
    __syncthreads();
    tree_best<DM_RED>(bv, bi, LowestMax{});
    const double sgn = (bi[0] < N && psi[(size_t)bi[0] * m + c] < 0.0) ? -1.0 : 1.0;     // (an all-NaN column: no index)
    const double scale = sqrt(-1.0 / lambda[c]);
    for (int n = threadIdx.x; n < N; n += DM_RED) {
        const double x = sgn * (psi[(size_t)n * m + c] / nrm);
        if (evecs) evecs[(size_t)n * m + c] = x;
        dmap[(size_t)n * m + c] = x * scale;
    }
}

}  // namespace pilot
