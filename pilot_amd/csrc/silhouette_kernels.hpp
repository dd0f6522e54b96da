// K18: the silhouette of every row of an n x D matrix under one label per row (sklearn.metrics.silhouette_samples), without the
// n x n distance matrix and without an n x n_clusters table.
//
// The rows are ordered by (label, original row) once (silhouette_gather_kernel), so a cluster is a run of consecutive corpus rows.
// silhouette_rows_kernel keeps one query per lane and sweeps that corpus with K16's knn_sweep: every lane is at the same corpus
// row at the same time, so a cluster boundary is wave-uniform and each lane carries just one running float64 sum.  At a boundary
// the sum of the finished cluster goes into a (the lane's own cluster) or into b = min(b, mean).  The distances are K16's
// (knn_chunk, knn_distance); a sum takes one add per member in ascending original row; no atomics, and nothing depends on the
// tile or grid geometry: the same call gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "knn_kernels.hpp"

namespace pilot {

// S (n x D, packed) = the rows order[0], order[1], ... of X (leading dimension ld); one element per thread
template <typename T>
__global__ void silhouette_gather_kernel(const T *__restrict__ X, long long ld, long long n, int D, const int *__restrict__ order,
                                         T *__restrict__ S) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * D) return;
    const long long p = e / D;
    const int d = (int)(e - p * D);
    S[e] = X[(long long)order[p] * ld + d];
}

// S: the n x D corpus in label order (packed); offsets: n_clusters + 1 entries, cluster c = rows offsets[c] .. offsets[c + 1] - 1,
// none empty; order[p]: the original row of corpus row p.  The query of lane t is corpus row q0 + blockIdx.x * KNN_THREADS + t;
// out[order[row]] = its silhouette.  metric as in knn_distance.
template <typename T, bool REGQ>
__global__ __launch_bounds__(KNN_THREADS, KNN_WAVES) void silhouette_rows_kernel(const T *__restrict__ S, int n, int D, int metric,
                                                                      const int *__restrict__ offsets, const int *__restrict__ order,
                                                                      int q0, double *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) T ys[KnnTile<T>::CAP];
    const long long qi = (long long)q0 + (long long)blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool active = qi < n;
    const long long row = active ? qi : 0;                     // an idle lane works on a valid row and keeps nothing

    int c = 0, c_begin = 0, c_end = offsets[1];                // the cluster the sweep is in: the same in every lane
    double sum = 0.0, a = 0.0, b = INFINITY;
    bool alone = false;
    knn_sweep<T, REGQ>(S, (long long)D, n, D, S + row * D, ys, [&](long long j0, const T *acc) {
#pragma unroll
        for (int p = 0; p < KNN_PB; ++p) {
            const long long j = j0 + p;
            if (j < n && j != row) sum += knn_distance(acc[p], metric);
            if (j + 1 == c_end) {                              // row j was the cluster's last: close its sum
                const int members = c_end - c_begin;
                if (row >= c_begin && row < c_end) {
                    alone = members == 1;
                    a = alone ? 0.0 : sum / (double)(members - 1);
                } else {
                    b = fmin(b, sum / (double)members);
                }
                sum = 0.0;
                c_begin = c_end;
                ++c;
                c_end = j + 1 < n ? offsets[c + 1] : -1;
            }
        }
    });
    if (!active) return;
    const double m = fmax(a, b);
    out[order[row]] = (alone || !(m > 0.0)) ? 0.0 : (b - a) / m;
}

}  // namespace pilot
