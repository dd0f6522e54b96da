// K1: the centroid cost matrix (C ABI: pilot_ot_cost_matrix*, include/pilot_ot.h).
#include <hip/hip_runtime.h>

#include <cmath>

#include "abi_common.hpp"

namespace {

// ------------------------------------------------------------------------------------------------
// K1: centroid cost matrix (scipy pdist + squareform, Trajectory.py:468-469).  K <= a few hundred,
// D <= a few hundred: one workgroup, one thread per unordered pair, fp64 like scipy.  Far below the
// size where an MFMA contraction pays (K*K*D = 75k FMAs at c3).
// aux: metric-specific extra input (mahalanobis: the D x D inverse covariance VI, computed by the host like scipy does)
__global__ void cost_matrix_kernel(const double *__restrict__ X, int K, int D, int metric, const double *__restrict__ aux,
                                   double *__restrict__ C) {
    extern __shared__ double stat[];  // per-row norm (cosine) or mean + centred norm (correlation); per-dimension variance (seuclidean)
    double *nrm = stat, *mean = stat + K, *var = stat + 2 * K;
    if (metric == PILOT_OT_METRIC_SEUCLIDEAN)       // scipy: V = np.var(X, axis=0, ddof=1)
        for (int d = threadIdx.x; d < D; d += blockDim.x) {
            double m = 0.0;
            for (int i = 0; i < K; ++i) m += X[(size_t)i * D + d];
            m /= K;
            double s = 0.0;
            for (int i = 0; i < K; ++i) { const double t = X[(size_t)i * D + d] - m; s += t * t; }
            var[d] = s / (K - 1);
        }
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        const double *x = X + (size_t)i * D;
        double m = 0.0;
        if (metric == PILOT_OT_METRIC_CORRELATION) {
            for (int d = 0; d < D; ++d) m += x[d];
            m /= D;
        }
        double s = 0.0;
        for (int d = 0; d < D; ++d) s += (x[d] - m) * (x[d] - m);
        mean[i] = m;
        nrm[i] = sqrt(s);
        C[(size_t)i * K + i] = 0.0;
    }
    __syncthreads();
    const int npairs = K * (K - 1) / 2;
    for (int pidx = threadIdx.x; pidx < npairs; pidx += blockDim.x) {
        // unrank (i < j) from the condensed pdist index
        int i = 0, rem = pidx;
        while (rem >= K - 1 - i) { rem -= K - 1 - i; ++i; }
        const int j = i + 1 + rem;
        const double *u = X + (size_t)i * D, *v = X + (size_t)j * D;
        double out = 0.0;
        switch (metric) {
        case PILOT_OT_METRIC_COSINE:
        case PILOT_OT_METRIC_CORRELATION: {
            const double mu = mean[i], mv = mean[j];
            double dot = 0.0;
            for (int d = 0; d < D; ++d) dot += (u[d] - mu) * (v[d] - mv);
            double c = dot / (nrm[i] * nrm[j]);
            if (fabs(c) > 1.0) c = copysign(1.0, c);  // scipy clips rounding overshoot
            out = 1.0 - c;
            break;
        }
        case PILOT_OT_METRIC_EUCLIDEAN:
        case PILOT_OT_METRIC_MINKOWSKI:          // scipy's default p = 2 (the reference forwards only the name)
        case PILOT_OT_METRIC_SQEUCLIDEAN: {
            double s = 0.0;
            for (int d = 0; d < D; ++d) { const double t = u[d] - v[d]; s += t * t; }
            out = metric == PILOT_OT_METRIC_SQEUCLIDEAN ? s : sqrt(s);
            break;
        }
        case PILOT_OT_METRIC_SEUCLIDEAN: {
            double s = 0.0;
            for (int d = 0; d < D; ++d) { const double t = u[d] - v[d]; s += t * t / var[d]; }
            out = sqrt(s);
            break;
        }
        case PILOT_OT_METRIC_BRAYCURTIS: {
            double s1 = 0.0, s2 = 0.0;
            for (int d = 0; d < D; ++d) { s1 += fabs(u[d] - v[d]); s2 += fabs(u[d] + v[d]); }
            out = s1 / s2;
            break;
        }
        case PILOT_OT_METRIC_CANBERRA: {
            double s = 0.0;
            for (int d = 0; d < D; ++d) {
                const double den = fabs(u[d]) + fabs(v[d]);
                if (den > 0.0) s += fabs(u[d] - v[d]) / den;          // 0/0 terms count as 0
            }
            out = s;
            break;
        }
        case PILOT_OT_METRIC_HAMMING: {
            int ne = 0;
            for (int d = 0; d < D; ++d) ne += u[d] != v[d];
            out = double(ne) / D;
            break;
        }
        case PILOT_OT_METRIC_CITYBLOCK: {
            double s = 0.0;
            for (int d = 0; d < D; ++d) s += fabs(u[d] - v[d]);
            out = s;
            break;
        }
        // scipy's "boolean" dissimilarities: pdist converts the rows to bool (non-zero = True) and counts agreements
        case PILOT_OT_METRIC_JACCARD: case PILOT_OT_METRIC_YULE: case PILOT_OT_METRIC_RUSSELLRAO: case PILOT_OT_METRIC_SOKALSNEATH:
        case PILOT_OT_METRIC_ROGERSTANIMOTO: case PILOT_OT_METRIC_SOKALMICHENER: case PILOT_OT_METRIC_KULCZYNSKI1: {
            double ntt = 0, ntf = 0, nft = 0, nff = 0;
            for (int d = 0; d < D; ++d) {
                const bool a = u[d] != 0.0, b = v[d] != 0.0;
                ntt += a && b; ntf += a && !b; nft += !a && b; nff += !a && !b;
            }
            const double R = ntf + nft;
            if (metric == PILOT_OT_METRIC_JACCARD) out = (ntt + R) > 0.0 ? R / (ntt + R) : 0.0;
            else if (metric == PILOT_OT_METRIC_YULE) { const double h = ntf * nft; out = h == 0.0 ? 0.0 : 2.0 * h / (ntt * nff + h); }
            else if (metric == PILOT_OT_METRIC_RUSSELLRAO) out = (double(D) - ntt) / double(D);
            else if (metric == PILOT_OT_METRIC_SOKALSNEATH) out = 2.0 * R / (ntt + 2.0 * R);
            else if (metric == PILOT_OT_METRIC_KULCZYNSKI1) out = ntt / R;
            else out = 2.0 * R / (ntt + nff + 2.0 * R);           // rogerstanimoto == sokalmichener
            break;
        }
        case PILOT_OT_METRIC_DICE: {            // (scipy evaluates this one on the values: ntt = sum u v, ...)
            double ntt = 0.0, nd = 0.0;
            for (int d = 0; d < D; ++d) { ntt += u[d] * v[d]; nd += u[d] * (1.0 - v[d]) + (1.0 - u[d]) * v[d]; }
            out = nd / (2.0 * ntt + nd);
            break;
        }
        case PILOT_OT_METRIC_JENSENSHANNON: {
            // no fused multiply-adds in this block: scipy's build (x86-64) rounds every product, and with proportional rows the sign of a
            // sum of +-1e-16 terms -- NaN or not -- follows those roundings (tools/ubench/rcp_f64.hip: m = (p + q) / 2 with p fused in)
#pragma clang fp contract(off)
            double su = 0.0, sv = 0.0;
            bool neg = false;
            for (int d = 0; d < D; ++d) { neg = neg || u[d] < 0.0 || v[d] < 0.0; su += u[d]; sv += v[d]; }
            if (neg || su == 0.0 || sv == 0.0) { out = HUGE_VAL; break; }     // (scipy: inf for a negative entry or an all-zero row)
            // (scipy's build multiplies by the reciprocals of the sums; dividing instead moves a Jensen-Shannon value near zero --
            // proportional rows -- by up to 1e-8 and turns scipy's NaN, the root of a sum that rounded below zero, into 0:
            // tools/fuzz_prepass.py, 20 000 pairs against scipy 1.15.3: 0 differences this way, 3 379 NaN mismatches the other)
            const double ru = 1.0 / su, rv = 1.0 / sv;
            double js = 0.0;
            for (int d = 0; d < D; ++d) {
                const double p = u[d] * ru, q = v[d] * rv, m = (p + q) / 2.0;
                if (p > 0.0) js += p * log(p / m);
                if (q > 0.0) js += q * log(q / m);
            }
            out = sqrt(js / 2.0);
            break;
        }
        case PILOT_OT_METRIC_MAHALANOBIS: {     // sqrt((u - v) VI (u - v)^T)
            double s = 0.0;
            for (int a = 0; a < D; ++a) {
                double t = 0.0;
                for (int b = 0; b < D; ++b) t += (u[b] - v[b]) * aux[(size_t)b * D + a];
                s += t * (u[a] - v[a]);
            }
            out = sqrt(s);
            break;
        }
        default: {  // chebyshev
            double s = 0.0;
            for (int d = 0; d < D; ++d) { const double t = fabs(u[d] - v[d]); s = t > s ? t : s; }
            out = s;
        }
        }
        C[(size_t)i * K + j] = out;
        C[(size_t)j * K + i] = out;
    }
}

}  // namespace

PILOT_API int pilot_ot_cost_matrix_dev_ex(const double *d_centroids, int K, int D, int metric, const double *d_aux, double *d_cost,
                                          void *stream) {
    if (!d_centroids || !d_cost) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (K <= 0 || D <= 0) return fail(PILOT_OT_EINVAL, "K=%d D=%d must be positive", K, D);
    if (metric < PILOT_OT_METRIC_COSINE || metric > PILOT_OT_METRIC_MAHALANOBIS)
        return fail(PILOT_OT_EINVAL, "unknown metric id %d", metric);
    if (metric == PILOT_OT_METRIC_MAHALANOBIS && !d_aux) return fail(PILOT_OT_EINVAL, "mahalanobis needs the D x D inverse covariance (aux)");
    if (K > 4096 || D > 4096) return fail(PILOT_OT_ENOTSUP, "K=%d D=%d: at most 4096 centroids / dimensions", K, D);
    const size_t lds = sizeof(double) * (2 * (size_t)K + D);     // beyond 64 KiB whenever 2 K + D > 8192 (at most 96 KiB)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(cost_matrix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(cost_matrix_kernel, dim3(1), dim3(1024), lds, static_cast<hipStream_t>(stream), d_centroids, K, D, metric, d_aux,
                       d_cost);
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_cost_matrix_dev(const double *d_centroids, int K, int D, int metric, double *d_cost, void *stream) {
    return pilot_ot_cost_matrix_dev_ex(d_centroids, K, D, metric, nullptr, d_cost, stream);
}

PILOT_API int pilot_ot_cost_matrix_ex(const double *centroids, int K, int D, int metric, const double *aux, double *cost) {
    if (!centroids || !cost) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (K <= 0 || D <= 0) return fail(PILOT_OT_EINVAL, "K=%d D=%d must be positive", K, D);
    const bool has_aux = metric == PILOT_OT_METRIC_MAHALANOBIS;
    if (has_aux && !aux) return fail(PILOT_OT_EINVAL, "mahalanobis needs the D x D inverse covariance (aux)");
    if (K > 4096 || D > 4096) return fail(PILOT_OT_ENOTSUP, "K=%d D=%d: at most 4096 centroids / dimensions", K, D);   // before any staging
    // staging from the calling thread's pool
    double *dx = nullptr, *dc = nullptr, *da = nullptr;
    HIP_TRY(pilot::ws(pilot::WS_COST_X, (size_t)K * D, &dx));
    HIP_TRY(pilot::ws(pilot::WS_COST_C, (size_t)K * K, &dc));
    HIP_TRY(hipMemcpy(dx, centroids, sizeof(double) * (size_t)K * D, hipMemcpyHostToDevice));
    if (has_aux) {
        HIP_TRY(pilot::ws(pilot::WS_COST_AUX, (size_t)D * D, &da));
        HIP_TRY(hipMemcpy(da, aux, sizeof(double) * (size_t)D * D, hipMemcpyHostToDevice));
    }
    const int rc = pilot_ot_cost_matrix_dev_ex(dx, K, D, metric, da, dc, nullptr);
    if (rc != PILOT_OT_OK) return rc;
    HIP_TRY(hipMemcpy(cost, dc, sizeof(double) * (size_t)K * K, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_cost_matrix(const double *centroids, int K, int D, int metric, double *cost) {
    return pilot_ot_cost_matrix_ex(centroids, K, D, metric, nullptr, cost);
}
