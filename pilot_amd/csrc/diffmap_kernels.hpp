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

namespace pilot {

constexpr int DM_TILE = 32;            // transpose tile of the symmetrisation
constexpr int DM_RED = 256;            // threads of the row-reduction / dot-product workgroups
constexpr int DM_FIN = 1024;           // threads of the single-workgroup step finish

// fixed-order sum over the workgroup (blockDim.x == NT, a power of two): every thread passes its partial, all get the total
template <int NT>
__device__ inline double dm_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// fixed-order sum over one wave (64 lanes, butterfly): every lane gets the total
__device__ inline double dm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

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
    s = dm_block_sum<DM_RED>(s, red);
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
    const double nrm = sqrt(dm_block_sum<DM_FIN>(s, red));
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
    s = dm_wave_sum(s);
    if (lane == 0) w[i] = s;
}

// h[k] = V[k] . w for k < nk: one workgroup (DM_RED threads) per basis vector
static __global__ void __launch_bounds__(DM_RED) lz_dots_kernel(const double *__restrict__ V, int N, const double *__restrict__ w,
                                                                double *__restrict__ h) {
    __shared__ double red[DM_RED];
    const double *vk = V + (size_t)blockIdx.x * N;
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += DM_RED) s += vk[n] * w[n];
    s = dm_block_sum<DM_RED>(s, red);
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

// End of Lanczos step j (basis V[0..j] holds j + 1 vectors, w = S v_j after the two Gram-Schmidt passes with coefficients h1, h2):
//   alpha[j] = h1[j] + h2[j];  beta[j] = |w|;  V[j + 1] = w / beta[j]  (when j + 1 < B).
// Breakdown (beta[j] <= tol: the Krylov space is invariant -- at step 0 always, since V[0] is an eigenvector): beta[j] = 0 and
// V[j + 1] is the next restart vector, orthogonalised against V[0..j] by two classical Gram-Schmidt passes and normalised; the
// restart count lives in *n_restart.  One workgroup of DM_FIN threads; w is overwritten.
static __global__ void __launch_bounds__(DM_FIN) lz_finish_kernel(double *__restrict__ V, int N, int j, int B, double *__restrict__ w,
                                                                  const double *__restrict__ h1, const double *__restrict__ h2,
                                                                  double tol, double *__restrict__ alpha, double *__restrict__ beta,
                                                                  int *__restrict__ n_restart) {
    __shared__ double red[DM_FIN];
    __shared__ double hs[1024];                               // (B <= 1024)
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += DM_FIN) s += w[n] * w[n];
    const double b = sqrt(dm_block_sum<DM_FIN>(s, red));
    if (threadIdx.x == 0) alpha[j] = h1[j] + h2[j];
    if (b > tol) {
        if (threadIdx.x == 0) beta[j] = b;
        if (j + 1 < B)
            for (int n = threadIdx.x; n < N; n += DM_FIN) V[(size_t)(j + 1) * N + n] = w[n] / b;
        return;
    }
    if (threadIdx.x == 0) beta[j] = 0.0;
    if (j + 1 >= B) return;                                   // (basis complete: nothing to continue with)
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
            t = dm_wave_sum(t);
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
    s = 0.0;
    for (int n = threadIdx.x; n < N; n += DM_FIN) s += w[n] * w[n];
    const double r = sqrt(dm_block_sum<DM_FIN>(s, red));
    for (int n = threadIdx.x; n < N; n += DM_FIN) V[(size_t)(j + 1) * N + n] = w[n] / r;
}

// Ritz vectors and the back-transform: psi[n][c] = dis[n] * sum_k Z[k][c] V[k][n] (k < nk, in order), c < m.  Z: nk x m row-major.
// psi: N x m row-major.  One thread per (n, c).
static __global__ void lz_ritz_kernel(const double *__restrict__ V, int N, int nk, const double *__restrict__ Z, int m,
                                      const double *__restrict__ dis, double *__restrict__ psi) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)N * m) return;
    const int n = (int)(t / m), c = (int)(t % m);
    double s = 0.0;
    for (int k = 0; k < nk; ++k) s += Z[(size_t)k * m + c] * V[(size_t)k * N + n];
    psi[t] = s * dis[n];
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
    const double nrm = sqrt(dm_block_sum<DM_RED>(s, red));
    bv[threadIdx.x] = best; bi[threadIdx.x] = at;
    __syncthreads();
    for (int st = DM_RED / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const double a = bv[threadIdx.x], b = bv[threadIdx.x + st];
            const int ia = bi[threadIdx.x], ib = bi[threadIdx.x + st];
            if (b > a || (b == a && ib < ia)) { bv[threadIdx.x] = b; bi[threadIdx.x] = ib; }
        }
        __syncthreads();
    }
    const double sgn = (bi[0] < N && psi[(size_t)bi[0] * m + c] < 0.0) ? -1.0 : 1.0;     // (an all-NaN column: no index)
    const double scale = sqrt(-1.0 / lambda[c]);
    for (int n = threadIdx.x; n < N; n += DM_RED) {
        const double x = sgn * (psi[(size_t)n * m + c] / nrm);
        if (evecs) evecs[(size_t)n * m + c] = x;
        dmap[(size_t)n * m + c] = x * scale;
    }
}

}  // namespace pilot
