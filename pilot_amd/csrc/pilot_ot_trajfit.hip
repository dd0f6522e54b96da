// C ABI of the trajectory model fits (include/pilot_ot.h, section "trajectory model fits"; kernels: trajfit_kernels.hpp).
// pilotpy's fit_best_model (tools/Cell_gene_selection.py) for all targets at once.  The host does the O(n) and 3 x 3 parts that
// every target shares -- the scaled time u, the Gram of [1, u, u^2] and the per-model matrices derived from it -- and moves the
// targets through the device in chunks of columns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "abi_common.hpp"
#include "trajfit_host.hpp"

namespace {

constexpr size_t CHUNK_BYTES = size_t(256) << 20;      // device copy of a host Y: at most this many bytes of columns at a time

// inverse of a small symmetric positive definite matrix (Gauss-Jordan with partial pivoting; k <= 3)
bool invert(int k, const double A[3][3], double X[3][3]) {
    double W[3][6] = {};
    for (int i = 0; i < k; ++i) {
        for (int j = 0; j < k; ++j) W[i][j] = A[i][j];
        W[i][k + i] = 1.0;
    }
    for (int c = 0; c < k; ++c) {
        int piv = c;
        for (int r = c + 1; r < k; ++r) if (std::fabs(W[r][c]) > std::fabs(W[piv][c])) piv = r;
        if (!(std::fabs(W[piv][c]) > 0.0)) return false;
        for (int j = 0; j < 2 * k; ++j) std::swap(W[c][j], W[piv][j]);
        const double d = W[c][c];
        for (int j = 0; j < 2 * k; ++j) W[c][j] /= d;
        for (int r = 0; r < k; ++r) {
            if (r == c) continue;
            const double f = W[r][c];
            for (int j = 0; j < 2 * k; ++j) W[r][j] -= f * W[c][j];
        }
    }
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) X[i][j] = W[i][k + j];
    return true;
}

// The shared part of a call: the time map (trajfit_host.hpp) and what depends on the Gram of [1, u, u^2]: per model G and vd,
// and the Pearson sum sxx; the range of x
int prepare(const double *x, int n, std::vector<double> &u, pilot::TrajfitArgs &a) {
    pilot::trajfit_time_map(x, n, u, a);
    double xmin = x[0], xmax = x[0];
    double mu[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i) {
        xmin = std::min(xmin, x[i]);
        xmax = std::max(xmax, x[i]);
        const double v = u[i];
        double p = 1.0;
        for (int k = 0; k < 5; ++k) { mu[k] += p; p *= v; }
    }
    const double ubar = mu[1] / n;
    double sxx = 0.0;
    for (int i = 0; i < n; ++i) sxx += (u[i] - ubar) * (u[i] - ubar);
    double G3[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G3[i][j] = mu[i + j];
    for (int md = 0; md < 3; ++md) {
        pilot::TrajfitModel &M = a.mod[md];
        const int p = md == 1 ? 3 : 2;
        const double (&C)[3][3] = M.C;
        double BB[3][3] = {}, H[3][3] = {};
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j)
                for (int k = 0; k < 3; ++k)
                    for (int l = 0; l < 3; ++l) BB[i][j] += C[k][i] * G3[k][l] * C[l][j];
        if (!invert(p, BB, H)) return fail(PILOT_OT_EINVAL, "x: the Gram matrix of the model features is singular");
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < 3; ++j)
                for (int k = 0; k < p; ++k) M.G[i][j] += H[i][k] * C[j][k];          // G = H C^T
        for (int j = 0; j < p; ++j) {
            double v = 0.0;
            for (int k = 0; k < p; ++k)
                for (int l = 0; l < p; ++l) v += M.R[j][k] * H[k][l] * M.R[j][l];
            M.vd[j] = v;                                                               // diag(R H R^T) = diag((Z^T Z)^-1)
        }
    }
    a.sxx = sxx;
    a.x_min = xmin;
    a.x_max = xmax;
    return PILOT_OT_OK;
}

int check_args(const void *Y, int dtype, int n, int n_targets, long long ld, const double *x, int model, double epsilon,
               double pval_thr, const pilot_ot_trajfit_out *out) {
    if (!Y || !x || !out) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n < 4) return fail(PILOT_OT_EINVAL, "n=%d: the fits need at least 4 observations", n);
    if (n_targets < 0) return fail(PILOT_OT_EINVAL, "n_targets=%d is negative", n_targets);
    if (int rc = pilot::check_ld(ld, n_targets)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (model != PILOT_OT_TRAJFIT_OLS && model != PILOT_OT_TRAJFIT_HUBER)
        return fail(PILOT_OT_EINVAL, "model=%d must be PILOT_OT_TRAJFIT_OLS or PILOT_OT_TRAJFIT_HUBER", model);
    if (!(epsilon >= 1.0) || !std::isfinite(epsilon)) return fail(PILOT_OT_EINVAL, "epsilon=%g must be finite and >= 1", epsilon);
    if (std::isnan(pval_thr)) return fail(PILOT_OT_EINVAL, "pval_thr is NaN");
    // three distinct times: with two, x^2 is affine in x and the linear_quadratic model has no unique fit
    double v1 = 0.0;
    int distinct = 1;
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(x[i])) return fail(PILOT_OT_EINVAL, "x[%d]=%g is not finite", i, x[i]);
        if (distinct == 1 && x[i] != x[0]) { v1 = x[i]; distinct = 2; }
        else if (distinct == 2 && x[i] != x[0] && x[i] != v1) distinct = 3;
    }
    if (distinct < 3) return fail(PILOT_OT_EINVAL, "x needs at least 3 distinct values (the linear_quadratic model), has %d", distinct);
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_trajectory_fits(const void *Y, int Y_is_device, int dtype, int n, int n_targets, long long ld, const double *x,
                                       int model, double epsilon, double pval_thr, int modify_r2, pilot_ot_trajfit_out *out,
                                       int *n_not_converged) {
    int rc = check_args(Y, dtype, n, n_targets, ld, x, model, epsilon, pval_thr, out);
    if (rc != PILOT_OT_OK) return rc;
    if (n_not_converged) *n_not_converged = 0;
    if (n_targets == 0) return PILOT_OT_OK;
    pilot::TrajfitArgs a;
    std::vector<double> u;
    rc = prepare(x, n, u, a);
    if (rc != PILOT_OT_OK) return rc;
    a.huber = model == PILOT_OT_TRAJFIT_HUBER;
    a.epsilon = epsilon;
    a.pval_thr = pval_thr;
    a.modify_r2 = modify_r2 != 0;
    a.max_iter = pilot::trajfit_max_iter();
    const size_t es = pilot::elem_size(dtype);
    long long tc = (long long)(CHUNK_BYTES / ((size_t)n * es)) / 64 * 64;
    if (const char *sw = pilot::test_switch("PILOT_OT_TRAJFIT_CHUNK_TARGETS")) {   // (tests: many chunks)
        const long long v = atoll(sw);
        if (v > 0) tc = (v + 63) / 64 * 64;
    }
    tc = std::max(tc, 64LL);
    tc = std::min(tc, ((long long)n_targets + 63) / 64 * 64);

    const double *d_u;
    const pilot::TrajfitArgs *d_args;
    double *d_out;
    rc = pilot::trajfit_stage(pilot::WS_TF_U, u, a, &d_u, &d_args);
    if (rc != PILOT_OT_OK) return rc;
    HIP_TRY(pilot::ws(pilot::WS_TF_OUT, (size_t)tc * pilot::TF_NOUT, &d_out));
    std::vector<double> rec((size_t)tc * pilot::TF_NOUT);
    int not_conv = 0;
    for (long long t0 = 0; t0 < n_targets; t0 += tc) {
        const int nt = (int)std::min<long long>(tc, n_targets - t0);
        const void *yc;                                          // a host Y: this chunk's columns, packed (the first chunk is the widest)
        long long ldc;
        rc = pilot::stage_dense(static_cast<const unsigned char *>(Y) + (size_t)t0 * es, Y_is_device, es, n, nt, ld, pilot::WS_TF_Y, &yc, &ldc);
        if (rc != PILOT_OT_OK) return rc;
        const unsigned blocks = (unsigned)((nt + 63) / 64);
        if (dtype == 0)
            hipLaunchKernelGGL(pilot::trajfit_kernel<float>, dim3(blocks), dim3(pilot::TF_BLOCK), 0, nullptr,
                               static_cast<const float *>(yc), ldc, nt, d_u, d_args, d_out);
        else
            hipLaunchKernelGGL(pilot::trajfit_kernel<double>, dim3(blocks), dim3(pilot::TF_BLOCK), 0, nullptr,
                               static_cast<const double *>(yc), ldc, nt, d_u, d_args, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(rec.data(), d_out, sizeof(double) * (size_t)nt * pilot::TF_NOUT, hipMemcpyDeviceToHost));
        for (int j = 0; j < nt; ++j) {
            const double *r = rec.data() + (size_t)j * pilot::TF_NOUT;
            const size_t t = (size_t)t0 + j;
            for (int k = 0; k < 9; ++k) {
                if (out->params) out->params[t * 9 + k] = r[pilot::TF_O_PARAMS + k];
                if (out->pvalues) out->pvalues[t * 9 + k] = r[pilot::TF_O_PVAL + k];
            }
            for (int m = 0; m < 3; ++m) {
                if (out->rsquared_adj) out->rsquared_adj[t * 3 + m] = r[pilot::TF_O_R2 + m];
                if (out->mod_rsquared_adj) out->mod_rsquared_adj[t * 3 + m] = r[pilot::TF_O_MR2 + m];
                if (out->sigma) out->sigma[t * 3 + m] = r[pilot::TF_O_SIGMA + m];
                if (out->steps) out->steps[t * 3 + m] = (int)r[pilot::TF_O_STEPS + m];
                if (out->flags) out->flags[t * 3 + m] = (int)r[pilot::TF_O_FLAGS + m];
                not_conv += ((int)r[pilot::TF_O_FLAGS + m] & PILOT_OT_TRAJFIT_NOT_CONVERGED) != 0;
            }
            if (out->chosen) out->chosen[t] = (int)r[pilot::TF_O_CHOSEN];
            if (out->slope) out->slope[t] = r[pilot::TF_O_SLOPE];
            if (out->pattern) out->pattern[t] = (int)r[pilot::TF_O_PATTERN];
            if (out->pearson_r) out->pearson_r[t] = r[pilot::TF_O_PR];
            if (out->pearson_p) out->pearson_p[t] = r[pilot::TF_O_PP];
            if (out->zero_fraction) out->zero_fraction[t] = r[pilot::TF_O_ZERO];
            if (out->mean) out->mean[t] = r[pilot::TF_O_MEAN];
        }
    }
    if (n_not_converged) *n_not_converged = not_conv;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_normalize_log1p(const void *X, int dtype, int n, int n_genes, double target_sum, const int *cols, int n_cols,
                                       void *out) {
    if (!X || !cols || !out) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n < 0 || n_genes < 1 || n_cols < 0) return fail(PILOT_OT_EINVAL, "n=%d, n_genes=%d, n_cols=%d", n, n_genes, n_cols);
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (!(target_sum > 0.0) || !std::isfinite(target_sum)) return fail(PILOT_OT_EINVAL, "target_sum=%g must be positive", target_sum);
    if (int rc = pilot::check_cols(cols, n_cols, n_genes)) return rc;
    if (n == 0 || n_cols == 0) return PILOT_OT_OK;
    const size_t es = pilot::elem_size(dtype);
    const long long rows = std::max<long long>(1, std::min<long long>(n, (long long)(CHUNK_BYTES / ((size_t)(n_genes + n_cols) * es))));
    unsigned char *d_x, *d_o;
    int *d_cols;
    HIP_TRY(pilot::ws(pilot::WS_TF_Y, (size_t)rows * n_genes * es, &d_x));
    HIP_TRY(pilot::ws(pilot::WS_TF_OUT, (size_t)rows * n_cols * es, &d_o));
    HIP_TRY(pilot::ws(pilot::WS_TF_COLS, (size_t)n_cols, &d_cols));
    HIP_TRY(hipMemcpy(d_cols, cols, sizeof(int) * n_cols, hipMemcpyHostToDevice));
    for (long long r0 = 0; r0 < n; r0 += rows) {
        const long long nr = std::min<long long>(rows, n - r0);
        HIP_TRY(hipMemcpy(d_x, static_cast<const unsigned char *>(X) + (size_t)r0 * n_genes * es, (size_t)nr * n_genes * es,
                          hipMemcpyHostToDevice));
        if (dtype == 0)
            hipLaunchKernelGGL(pilot::trajfit_normalize_kernel<float>, dim3((unsigned)nr), dim3(pilot::TF_NORM_THREADS), 0, nullptr,
                               reinterpret_cast<const float *>(d_x), n_genes, d_cols, n_cols, target_sum, reinterpret_cast<float *>(d_o));
        else
            hipLaunchKernelGGL(pilot::trajfit_normalize_kernel<double>, dim3((unsigned)nr), dim3(pilot::TF_NORM_THREADS), 0, nullptr,
                               reinterpret_cast<const double *>(d_x), n_genes, d_cols, n_cols, target_sum, reinterpret_cast<double *>(d_o));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(static_cast<unsigned char *>(out) + (size_t)r0 * n_cols * es, d_o, (size_t)nr * n_cols * es,
                          hipMemcpyDeviceToHost));
    }
    return PILOT_OT_OK;
}
