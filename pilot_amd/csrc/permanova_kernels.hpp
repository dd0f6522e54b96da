// K29: PERMANOVA of a distance matrix (Anderson 2001), the rule of DESIGN.md "K29".  Four kernels:
//   pm_prepare_kernel   gathers the used rows of D, symmetrises, squares: A_ij = -0.5 s_ij s_ij (s_ii = 0), written into an NP x NP
//                       image (NP = n rounded up to PM_RB, the pad is zero) with its row sums; a non-finite entry is reported
//                       through an integer atomicMin.  pm_total_kernel adds the row sums in a fixed order.
//   pm_permute_kernel   one workgroup per permutation b: Philox4x32-10 keys, the (stratum, key, index) records sorted in LDS by
//                       K21's bitonic network (rs_bitonic_lds), the permutation written as int32.  b = 0 is the identity.
//   pm_quad_kernel      the quadratic forms z^T A z of the columns of a chunk of permutations, flattened over (permutation, column)
//                       and tiled 16 wide.  A workgroup of 4 waves owns PM_CT column tiles and one block of PM_RB rows of A: it
//                       gathers Z[k, col] = Q[perm[k], c] into LDS PM_KC rows of k at a time, every wave accumulates
//                       T = A Z for its PM_R row tiles on v_mfma_f64_16x16x4_f64, multiplies by Z elementwise and the workgroup
//                       reduces per column in a fixed order.  A is symmetric bit for bit, so the A operand (row i, step k) is read
//                       as A[k][i]: 16 adjacent doubles per lane group.
//   pm_terms_kernel     per (permutation, term): the row blocks' partial sums of a column in block order, then the term's columns
//                       in column order.
// A column's value depends on n, A and that column of Z alone: not on where in a tile, a chunk or a call it sits (an MFMA output
// column is a k-ordered fma chain over its own B column), so permutation b has the same bits under any batching.  No
// floating-point atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include "rank_sums_kernels.hpp"     // rs_bitonic_lds, rs_u64
#include "reduce.hpp"

namespace pilot {

constexpr int PM_MAX_N = 8192;        // the LDS sort: 8192 records of 16 B = 128 KiB
constexpr int PM_MAX_COLS = 4096;     // columns of Q
constexpr int PM_CHUNK_PERMS = 4096;  // permutations per pass (test switch PILOT_OT_PERMANOVA_CHUNK lowers it)
constexpr int PM_CHUNK_COLS = 65536;  // and columns per pass: chunk = min(PM_CHUNK_PERMS, PM_CHUNK_COLS / c)
constexpr int PM_THREADS = 256;
constexpr int PM_CT = 2;              // column tiles per workgroup: one read of A serves 32 columns
constexpr int PM_R = 2;               // row tiles per wave
constexpr int PM_RB = 4 * PM_R * 16;  // rows of A per workgroup
constexpr int PM_KC = 64;             // rows of Z per LDS chunk
constexpr int PM_ZLD = PM_KC + 2;     // LDS stride of a column of Z: the 16 columns x 2 lane groups of a half wave hit 64 banks
constexpr int PM_COLS = 16 * PM_CT;
constexpr rs_u64 PM_NO_BAD = ~0ull;

// ---- Philox4x32-10 (Salmon et al. 2011), the published constants ---------------------------------------------------------------
__host__ __device__ inline void pm_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned *out) {
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct PmRec {
    rs_u64 key;
    unsigned stratum, idx;
    __device__ bool operator>(const PmRec &o) const {
        if (stratum != o.stratum) return stratum > o.stratum;
        if (key != o.key) return key > o.key;
        return idx > o.idx;
    }
};
struct PmSortKey {
    typedef PmRec Rec;
    __device__ static const PmRec &value(const PmRec &r) { return r; }
};

// Grid: `count` workgroups, permutation b = start + blockIdx.x.  Dynamic LDS: P records, P the power of two >= n.
// strata[i] >= 0; rorder: the rows ordered by (stratum, i).  perm: count x n.
__global__ void __launch_bounds__(PM_THREADS) pm_permute_kernel(int n, int P, const int *__restrict__ strata, const int *__restrict__ rorder,
                                                               rs_u64 seed, long long start, int *__restrict__ perm) {
    extern __shared__ __attribute__((aligned(16))) char pm_lds[];
    PmRec *s = reinterpret_cast<PmRec *>(pm_lds);
    const long long b = start + blockIdx.x;
    int *out = perm + (size_t)blockIdx.x * n;
    if (b == 0) {
        for (int i = threadIdx.x; i < n; i += PM_THREADS) out[i] = i;
        return;
    }
    for (int p = threadIdx.x; p < P; p += PM_THREADS) {
        PmRec r{~0ull, ~0u, (unsigned)p};
        if (p < n) {
            unsigned w[4];
            pm_philox((unsigned)p, (unsigned)(b & 0xFFFFFFFFll), (unsigned)((rs_u64)b >> 32), 0u, (unsigned)(seed & 0xFFFFFFFFull),
                      (unsigned)(seed >> 32), w);
            r.key = ((rs_u64)w[0] << 32) | w[1];
            r.stratum = (unsigned)strata[p];
        }
        s[p] = r;
    }
    __syncthreads();
    rs_bitonic_lds<PmSortKey, PM_THREADS>(s, P, 0, 2, P);
    for (int t = threadIdx.x; t < n; t += PM_THREADS) out[rorder[t]] = (int)s[t].idx;
}

// Grid: NP workgroups (row i of the image).  rows: the n used rows of D, or nullptr for all of them.
template <typename T>
__global__ void __launch_bounds__(PM_THREADS) pm_prepare_kernel(const T *__restrict__ D, long long ld, const int *__restrict__ rows, int n,
                                                               int NP, double *__restrict__ A, double *__restrict__ rowsum, rs_u64 *bad) {
    __shared__ double red[PM_THREADS / 64];
    const int i = blockIdx.x;
    const long long ri = i < n ? (rows ? rows[i] : i) : 0;
    double part = 0.0;
    for (int j = threadIdx.x; j < NP; j += PM_THREADS) {
        double a = 0.0;
        if (i < n && j < n && j != i) {
            const long long rj = rows ? rows[j] : j;
            const double dij = (double)D[ri * ld + rj], dji = (double)D[rj * ld + ri];
            if (!__builtin_isfinite(dij)) atomicMin(bad, ((rs_u64)ri << 32) | (rs_u64)rj);
            const double sij = (dij + dji) / 2.0;
            a = (-0.5 * sij) * sij;
            part += a;
        }
        A[(size_t)i * NP + j] = a;
    }
    const double tot = block_sum<PM_THREADS / 64>(part, red);
    if (threadIdx.x == 0) rowsum[i] = tot;
}

// One workgroup: total[0] = the sum of rowsum[0 .. n), thread-strided partials then the fixed-order workgroup sum.
__global__ void __launch_bounds__(PM_THREADS) pm_total_kernel(const double *__restrict__ rowsum, int n, double *__restrict__ total) {
    __shared__ double red[PM_THREADS / 64];
    double part = 0.0;
    for (int i = threadIdx.x; i < n; i += PM_THREADS) part += rowsum[i];
    const double tot = block_sum<PM_THREADS / 64>(part, red);
    if (threadIdx.x == 0) total[0] = tot;
}

// Z[row, flattened column fc] of the chunk: column cc of Q, permuted by permutation pb of the chunk
__device__ inline double pm_z(const double *__restrict__ Q, int c, const int *__restrict__ perm, int n, int row, long long pb, int cc, bool live) {
    return live && row < n ? Q[(size_t)perm[pb * n + row] * c + cc] : 0.0;
}

// Grid: (ceil(ncols / PM_COLS), NP / PM_RB).  partial: (NP / PM_RB) x ncols_pad, ncols_pad = gridDim.x * PM_COLS.
__global__ void __launch_bounds__(PM_THREADS) pm_quad_kernel(const double *__restrict__ A, int NP, int n, const double *__restrict__ Q, int c,
                                                            const int *__restrict__ perm, long long ncols, double *__restrict__ partial,
                                                            long long ncols_pad) {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    __shared__ double zs[PM_COLS * PM_ZLD];
    __shared__ double red[4 * PM_CT * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lg = lane >> 4;
    const long long fc0 = (long long)blockIdx.x * PM_COLS;
    const int row0 = blockIdx.y * PM_RB + wave * PM_R * 16;
    // the gather's column of this thread: k = lane, columns wave, wave + 4, ...
    acc_t acc[PM_R][PM_CT];
#pragma unroll
    for (int r = 0; r < PM_R; ++r)
#pragma unroll
        for (int t = 0; t < PM_CT; ++t) acc[r][t] = acc_t{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < NP; k0 += PM_KC) {
        __syncthreads();                       // the last chunk's readers are done
#pragma unroll
        for (int j = 0; j < PM_COLS / 4; ++j) {
            const int col = wave + 4 * j;
            const long long fc = fc0 + col;
            zs[col * PM_ZLD + lane] = pm_z(Q, c, perm, n, k0 + lane, fc / c, (int)(fc % c), fc < ncols);
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < PM_KC / 4; ++kk) {
            const int k = kk * 4 + lg;
            double a[PM_R], z[PM_CT];
#pragma unroll
            for (int r = 0; r < PM_R; ++r) a[r] = A[(size_t)(k0 + k) * NP + row0 + r * 16 + lc];      // A[i][k] = A[k][i]
#pragma unroll
            for (int t = 0; t < PM_CT; ++t) z[t] = zs[(t * 16 + lc) * PM_ZLD + k];
#pragma unroll
            for (int r = 0; r < PM_R; ++r)
#pragma unroll
                for (int t = 0; t < PM_CT; ++t) acc[r][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], z[t], acc[r][t], 0, 0, 0);
        }
    }
    // the f64 MFMA's own C/D map: column = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int t = 0; t < PM_CT; ++t) {
        const long long fc = fc0 + t * 16 + lc;
        const long long pb = fc / c;
        const int cc = (int)(fc % c);
        double p = 0.0;
#pragma unroll
        for (int r = 0; r < PM_R; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) p += pm_z(Q, c, perm, n, row0 + r * 16 + lg + 4 * g, pb, cc, fc < ncols) * acc[r][t][g];
        red[(wave * PM_CT + t) * 64 + lane] = p;
    }
    __syncthreads();
    if (tid < PM_COLS) {
        const int t = tid >> 4, col = tid & 15;
        double s = 0.0;
        for (int w = 0; w < 4; ++w)
            for (int g = 0; g < 4; ++g) s += red[(w * PM_CT + t) * 64 + g * 16 + col];
        partial[(size_t)blockIdx.y * ncols_pad + fc0 + tid] = s;
    }
}

// One thread per (permutation of the chunk, term): term_off[t] .. term_off[t + 1] are the term's columns.
__global__ void pm_terms_kernel(const double *__restrict__ partial, long long ncols_pad, int n_blocks, int c, const int *__restrict__ term_off,
                                int n_terms, long long count, double *__restrict__ ss) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= count * n_terms) return;
    const long long b = id / n_terms;
    const int t = (int)(id % n_terms);
    double s = 0.0;
    for (int col = term_off[t]; col < term_off[t + 1]; ++col) {
        double v = 0.0;
        for (int rb = 0; rb < n_blocks; ++rb) v += partial[(size_t)rb * ncols_pad + b * c + col];
        s += v;
    }
    ss[id] = s;
}

}  // namespace pilot
