// K16: the exact k-nearest-neighbour graph of the rows of an n x D matrix (the cells of an embedding); the per-row part of UMAP's
// fuzzy simplicial set is in knn_smooth_kernel.hpp.  The n x n distance matrix is never formed.
//
// knn_rows_kernel: one query row per lane, corpus rows staged through LDS in tiles and read back as wave-wide broadcasts.  A squared
// distance is the direct sum over d of (x_d - y_d)^2 in the element type T, d ascending, one fused multiply-add per term; the corpus is
// scanned in ascending row order and a candidate enters a query's list only if it is strictly closer than the list's k-th, behind
// every entry at the same distance, so a list is ordered by (distance, index).  No atomics: the same call gives the same bits.
// knn_sweep is that walk over the corpus with the per-sub-tile step left to the caller; K18 (silhouette_kernels.hpp) runs on it too.
#pragma once
#include <hip/hip_runtime.h>


namespace pilot {

constexpr int KNN_THREADS = 256;             // queries per block, one per lane
constexpr int KNN_PB = 16;                   // corpus points per register block: one accumulator each
constexpr int KNN_DC = 16;                   // dims per unrolled chunk
constexpr int KNN_REGQ_D = 64;               // D up to here: the whole query row lives in registers
constexpr int KNN_LDS_BYTES = 32 * 1024;     // the staged corpus tile
constexpr int KNN_GRID_MAX = 4096;           // query blocks per launch (the host loops over longer query ranges)
constexpr int KNN_WAVES = 2;                 // per SIMD: the query (64 dims), 16 accumulators and the LDS reads the compiler keeps in
                                             // flight take about 250 (float32) / 200 (float64) registers; at 168 or 128 it spills

// The corpus tile in LDS: `ns` sub-tiles of KNN_PB points, each holding `dl` dims; element (sub-tile s, dim dd, point p) sits at
// (s * dl + dd) * KNN_PB + p, so the KNN_PB values of one dim are contiguous and every lane reads the same address (a broadcast).
// When all dims (padded to KNN_DC) fit beside at least one sub-tile, dl = Dpad and the tile holds as many sub-tiles as fit;
// otherwise the tile is one sub-tile and the dims pass through in groups of dl.
template <typename T> struct KnnTile {
    static constexpr int CAP = KNN_LDS_BYTES / (int)sizeof(T);
    int Dpad, dl, ns;
    __host__ __device__ explicit KnnTile(int D) {
        Dpad = (D + KNN_DC - 1) / KNN_DC * KNN_DC;
        dl = Dpad < CAP / KNN_PB ? Dpad : CAP / KNN_PB;
        ns = Dpad <= dl ? CAP / (KNN_PB * Dpad) : 1;
    }
};

// acc[p] += (q[c] - y[c][p])^2 over one chunk of KNN_DC dims; yc: the chunk's first dim in the LDS tile
template <typename T> __device__ __forceinline__ void knn_chunk(const T *q, const T *yc, T *acc) {
#pragma unroll
    for (int c = 0; c < KNN_DC; ++c) {
        const T qv = q[c];
#pragma unroll
        for (int p = 0; p < KNN_PB; ++p) {
            const T df = qv - yc[c * KNN_PB + p];
            acc[p] = fma(df, df, acc[p]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);       // the next chunk's LDS reads stay behind this one: without it they all go first and spill
}

// (d, j) into one query's list (entry c at bd[c * m], bi[c * m]): behind every entry with a distance <= d.  j arrives in ascending
// order, so equal distances keep ascending indices.
template <typename T> __device__ __forceinline__ void knn_insert(T *bd, int *bi, size_t m, int k, int &cnt, T &kth, T d, int j) {
    int pos = cnt < k ? cnt : k - 1;
    while (pos > 0 && bd[(size_t)(pos - 1) * m] > d) {
        bd[(size_t)pos * m] = bd[(size_t)(pos - 1) * m];
        bi[(size_t)pos * m] = bi[(size_t)(pos - 1) * m];
        --pos;
    }
    bd[(size_t)pos * m] = d;
    bi[(size_t)pos * m] = j;
    if (cnt < k) ++cnt;
    if (cnt == k) kth = bd[(size_t)(k - 1) * m];
}

// One query (the row xq of D dims) against all n rows of X (leading dimension ld), by every lane of the block at once: the corpus
// goes through the LDS tile ys (KnnTile<T>::CAP elements) in ascending row order and each(j0, acc) is called for every sub-tile
// with acc[p] = the squared distance to corpus row j0 + p (rows past n: to a row of zeros).  Every lane is at the same corpus row
// at the same time.  REGQ: D <= KNN_REGQ_D and the query stays in registers; otherwise any D, and a query chunk is read again
// from xq for every sub-tile.
template <typename T, bool REGQ, typename F>
__device__ __forceinline__ void knn_sweep(const T *__restrict__ X, long long ld, int n, int D, const T *xq, T *ys, F &&each) {
    const KnnTile<T> tile(D);
    const int dl_max = tile.dl, ns = tile.ns, tp = ns * KNN_PB;
    T q[REGQ ? KNN_REGQ_D : KNN_DC];
    if constexpr (REGQ) {
#pragma unroll
        for (int d = 0; d < KNN_REGQ_D; ++d) q[d] = d < D ? xq[d] : T(0);
    }
    T acc[KNN_PB];

    for (long long t0 = 0; t0 < n; t0 += tp) {
        for (int dg = 0; dg < tile.Dpad; dg += dl_max) {
            const int dl = tile.Dpad - dg < dl_max ? tile.Dpad - dg : dl_max;      // a multiple of KNN_DC
            __syncthreads();
            // point fastest: a wave's stores go to consecutive banks; rows past n and dims past D are zeros
            for (int e = threadIdx.x; e < tp * dl; e += KNN_THREADS) {
                const int pt = e % tp, dd = e / tp;
                const long long j = t0 + pt;
                const int d = dg + dd;
                ys[((pt / KNN_PB) * dl + dd) * KNN_PB + pt % KNN_PB] = (j < n && d < D) ? X[j * ld + d] : T(0);
            }
            __syncthreads();
            const bool last = dg + dl >= tile.Dpad;
            for (int s = 0; s < ns; ++s) {
                const long long j0 = t0 + (long long)s * KNN_PB;
                if (j0 >= n) break;
                if (dg == 0) {
#pragma unroll
                    for (int p = 0; p < KNN_PB; ++p) acc[p] = T(0);
                }
                const T *yt = ys + s * dl * KNN_PB;
                if constexpr (REGQ) {
#pragma unroll
                    for (int ch = 0; ch < KNN_REGQ_D / KNN_DC; ++ch)
                        if (ch * KNN_DC < dl) knn_chunk(q + ch * KNN_DC, yt + ch * KNN_DC * KNN_PB, acc);
                } else {
                    for (int ch = 0; ch < dl / KNN_DC; ++ch) {
#pragma unroll
                        for (int c = 0; c < KNN_DC; ++c) {
                            const int d = dg + ch * KNN_DC + c;
                            q[c] = d < D ? xq[d] : T(0);
                        }
                        knn_chunk(q, yt + ch * KNN_DC * KNN_PB, acc);
                    }
                }
                if (last) each(j0, acc);
            }
        }
    }
}

// the distance of a finished sum of squares, formed in f64: its square root (metric 0) or half of it (metric 1: between unit rows)
template <typename T> __device__ __forceinline__ double knn_distance(T sum, int metric) {
    const double s = (double)sum;
    return metric == 0 ? sqrt(s) : 0.5 * s;
}

// Queries q0 + blockIdx.x * KNN_THREADS + lane of the m query rows row_begin .. row_begin + m against all n rows of X (leading
// dimension ld).  best_d / best_i: k x m scratch lists (lane-contiguous).  out_i / out_d: m x k row-major; out_d = knn_distance of
// the sum.  REGQ: as in knn_sweep.
template <typename T, bool REGQ>
__global__ __launch_bounds__(KNN_THREADS, KNN_WAVES) void knn_rows_kernel(const T *__restrict__ X, long long ld, int n, int D, int k, int metric,
                                                               long long row_begin, int m, int q0, T *__restrict__ best_d,
                                                               int *__restrict__ best_i, int *__restrict__ out_i,
                                                               double *__restrict__ out_d) {
    __shared__ __attribute__((aligned(16))) T ys[KnnTile<T>::CAP];
    const long long qi = (long long)q0 + (long long)blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool active = qi < m;
    const long long row = row_begin + (active ? qi : 0);       // an idle lane works on a valid row and keeps nothing
    T *bd = best_d + (active ? qi : 0);
    int *bi = best_i + (active ? qi : 0);
    T kth = T(0);
    int cnt = 0;

    knn_sweep<T, REGQ>(X, ld, n, D, X + row * ld, ys, [&](long long j0, const T *acc) {
#pragma unroll
        for (int p = 0; p < KNN_PB; ++p) {
            const long long j = j0 + p;
            const T d = acc[p];
            if (active && j < n && j != row && (cnt < k || d < kth)) knn_insert(bd, bi, (size_t)m, k, cnt, kth, d, (int)j);
        }
    });
    if (!active) return;
    for (int c = 0; c < k; ++c) {
        out_i[(size_t)qi * k + c] = bi[(size_t)c * m];
        out_d[(size_t)qi * k + c] = knn_distance(bd[(size_t)c * m], metric);
    }
}

// sum_d x_d^2 of a row in f64, d ascending, every product and sum rounded on its own (no contraction: the host restatement forms
// the same bits); *finite: every element is
template <typename T> __device__ inline double knn_row_ssq(const T *x, int D, bool *finite) {
    double s = 0.0;
    bool ok = true;
    for (int d = 0; d < D; ++d) {
        const double v = (double)x[d];
        ok &= isfinite(v);
        s = __dadd_rn(s, __dmul_rn(v, v));
    }
    *finite = ok;
    return s;
}

// flags[0]: the first row with a non-finite element (under cosine also: whose f64 sum of squares overflows); flags[1], cosine only:
// the first row whose sum of squares is 0.  INT_MAX: none.  One row per thread; the integer minimum does not depend on the order.
template <typename T> __global__ void knn_check_kernel(const T *__restrict__ X, long long ld, int n, int D, int metric, int *flags) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool finite;
    const double s = knn_row_ssq(X + i * ld, D, &finite);
    if (!finite || (metric == 1 && isinf(s)))
        atomicMin(&flags[0], (int)i);
    else if (metric == 1 && s == 0.0)
        atomicMin(&flags[1], (int)i);
}

// U (n x D, packed) = every row of X divided by its f64 norm, the quotient formed in f64 and rounded to T
template <typename T> __global__ void knn_normalize_kernel(const T *__restrict__ X, long long ld, int n, int D, T *__restrict__ U) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool finite;
    const T *x = X + i * ld;
    const double norm = sqrt(knn_row_ssq(x, D, &finite));
    for (int d = 0; d < D; ++d) U[i * D + d] = (T)((double)x[d] / norm);
}

}  // namespace pilot
