// C ABI of the principal components (include/pilot_ot.h, section "principal components"; kernels: pca_kernels.hpp, the Lanczos
// step: lanczos_host.hpp).  The matrix is a sparse handle (row and column form in HBM) or a dense row-major one on the host or in
// HBM; cols and the results are host arrays.  The column moments come from the group-moments entry points (one group), the small
// tridiagonal Ritz problem is solved on the host, so the calls synchronise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <limits>
#include <vector>

#include "abi_common.hpp"
#include "csr_handle.hpp"
#include "lanczos_host.hpp"
#include "pca_kernels.hpp"

namespace {

struct Operator {
    long long n;
    int D;
    const double *sbar;                                        // device, D
    std::function<void(const double *v, const double *dot, double *t)> forward;             // t = S v - dot[0]
    std::function<void(const double *t, const double *part, double *w)> transposed;         // w = S^T t - sbar (1 . t)
    std::function<void(const double *Vm, int k, const double *off, double *out)> scores;    // out = S Vm - 1 off^T
};

// what can be judged without the values: PILOT_OT_EINVAL before any HIP call
int check_args(long long n, int n_cols_total, const int *cols, int n_sel, int scale, double max_value, int n_comps) {
    if (scale != 0 && scale != 1) return fail(PILOT_OT_EINVAL, "scale=%d must be 0 or 1", scale);
    if (!(max_value > 0.0)) return fail(PILOT_OT_EINVAL, "max_value=%g must be positive (INFINITY: no clip)", max_value);
    if (int rc = pilot::check_cols(cols, n_sel, n_cols_total)) return rc;
    if (cols) {
        std::vector<int> at((size_t)n_cols_total, -1);
        for (int j = 0; j < n_sel; ++j) {
            if (at[cols[j]] >= 0) return fail(PILOT_OT_EINVAL, "cols[%d]=%d repeats cols[%d]", j, cols[j], at[cols[j]]);
            at[cols[j]] = j;
        }
    }
    if (n < 2) return fail(PILOT_OT_EINVAL, "n=%lld: principal components need at least 2 rows", n);
    if (n > INT_MAX) return fail(PILOT_OT_ENOTSUP, "n=%lld rows need more than 32-bit row indices", n);
    const long long cap = std::min<long long>({n - 1, (long long)n_sel - 1, (long long)pilot::LZ_MAX_EVECS});
    if (n_comps < 1 || n_comps > cap)
        return fail(PILOT_OT_EINVAL, "n_comps=%d outside [1, min(n - 1, columns - 1, %d)] = [1, %lld]", n_comps, pilot::LZ_MAX_EVECS, cap);
    return PILOT_OT_OK;
}

int check_finite(const std::vector<double> &mean, const std::vector<double> &m2) {
    for (size_t j = 0; j < mean.size(); ++j)
        if (!std::isfinite(mean[j]) || !std::isfinite(m2[j]))
            return fail(PILOT_OT_EINVAL, "selected column %zu holds a non-finite value", j);
    return PILOT_OT_OK;
}

// The eigenpairs of A = Zc^T Zc by Lanczos and everything behind them.  ssq (host, D): sum_i (z_ij - zbar_j)^2 per column.
int solve(const Operator &op, const std::vector<double> &ssq, int k, double *scores, double *pcs, double *variance, double *ratio, int *info) {
    const long long n = op.n;
    const int D = op.D;
    double trace = 0.0;
    for (int j = 0; j < D; ++j) trace += ssq[j];               // = trace(A) >= lambda_0: the scale of the two tolerances
    info[0] = 0;
    info[1] = 0;
    if (!(trace > 0.0)) {                                      // every selected column is constant: A = 0
        std::fill(scores, scores + (size_t)n * k, 0.0);
        std::fill(pcs, pcs + (size_t)D * k, 0.0);
        std::fill(variance, variance + k, 0.0);
        std::fill(ratio, ratio + k, 0.0);
        info[1] = PILOT_OT_PCA_RANK_DEFICIENT;
        return PILOT_OT_OK;
    }
    int B = std::min(D, pilot::LZ_MAX_BASIS);
    if (const char *sw = pilot::test_switch("PILOT_OT_PCA_BASIS")) {          // (tests: a basis too small to converge)
        const int b = atoi(sw);
        if (b > 0 && b < B) B = b;
    }
    B = std::max(B, k);
    hipStream_t s = nullptr;

    double *V, *vec, *Zs, *d_pcs, *d_scores;
    HIP_TRY(pilot::ws(pilot::WS_PCA_V, (size_t)B * D, &V));
    HIP_TRY(pilot::ws(pilot::WS_PCA_VEC, (size_t)D + (size_t)n + 4 * (size_t)B + pilot::PCA_SUM_BLOCKS + pilot::LZ_MAX_EVECS + 2, &vec));
    HIP_TRY(pilot::ws(pilot::WS_PCA_Z, (size_t)B * k, &Zs));
    HIP_TRY(pilot::ws(pilot::WS_PCA_PCS, (size_t)D * k, &d_pcs));
    HIP_TRY(pilot::ws(pilot::WS_PCA_SCORES, (size_t)n * k, &d_scores));
    double *w = vec, *t = w + D, *h1 = t + n, *h2 = h1 + B, *al = h2 + B, *be = al + B;
    double *part = be + B, *off = part + pilot::PCA_SUM_BLOCKS, *dot = off + pilot::LZ_MAX_EVECS;
    int *n_restart = reinterpret_cast<int *>(dot + 1);

    hipLaunchKernelGGL(pilot::pca_start_kernel, dim3(1), dim3(pilot::DM_FIN), 0, s, D, V);
    HIP_TRY(hipMemsetAsync(n_restart, 0, sizeof(int), s));
    HIP_TRY(hipGetLastError());

    // Lanczos (lanczos_run: the steps, the look at T every LZ_CHECK_EVERY steps from step k on, and the acceptance rule).  A
    // breakdown means that the Krylov space of the start vector is invariant: its Ritz pairs are eigenpairs, but it holds only one
    // direction per distinct eigenvalue, so a breakdown, like k converged pairs, only begins the verification block; the steps of
    // that block are not part of the result unless it found something and the basis went on to become complete.
    pilot::LanczosSpec spec;
    spec.N = D;
    spec.B = B;
    spec.want = k;
    spec.breakdown = pilot::LZ_BREAKDOWN_TOL * trace;
    spec.norm = 0.0;                                           // tolerances relative to the leading Ritz value
    spec.floor_rel = (double)D * std::numeric_limits<double>::epsilon();
    spec.start_is_eigenvector = false;
    pilot::LanczosRun run;
    HIP_TRY(pilot::lanczos_run(spec, V, w, h1, h2, al, be, n_restart, s, [&](const double *vj, double *wj) {
        hipLaunchKernelGGL(pilot::pca_dot_kernel, dim3(1), dim3(pilot::DM_FIN), 0, s, op.sbar, vj, D, dot);
        op.forward(vj, dot, t);
        hipLaunchKernelGGL(pilot::pca_sum_kernel, dim3(pilot::PCA_SUM_BLOCKS), dim3(256), 0, s, t, n, part);
        op.transposed(t, part, wj);
    }, &run));
    const std::vector<double> &ha = run.ha, &hb = run.hb;
    const int steps = run.steps;
    const bool converged = run.converged;
    std::vector<double> d, e, z;

    // the Ritz pairs of the final basis: eigenvectors of T as columns
    const int nk = run.nk, have = std::min(k, nk);
    d.assign(ha.begin(), ha.begin() + nk);
    e.assign(hb.begin(), hb.begin() + nk);
    z.assign((size_t)nk * nk, 0.0);
    for (int q = 0; q < nk; ++q) z[(size_t)q * nk + q] = 1.0;
    if (!pilot::tridiag_ql(nk, d.data(), e.data(), z.data(), nk)) return fail(PILOT_OT_EHIP, "tridiagonal QL did not converge (%d steps)", nk);
    const std::vector<int> ix = pilot::order_desc(d);
    const double lam0 = d[ix[0]], floor = (double)D * std::numeric_limits<double>::epsilon() * lam0;
    const double total_var = trace / (double)(n - 1);
    bool deficient = nk < k;                                   // a breakdown before k pairs
    std::vector<double> zs((size_t)nk * k, 0.0);
    for (int c = 0; c < k; ++c) {
        const double lam = c < have ? d[ix[c]] : 0.0;
        deficient |= !(lam > floor);
        variance[c] = lam / (double)(n - 1);
        ratio[c] = variance[c] / total_var;
        for (int q = 0; c < have && q < nk; ++q) zs[(size_t)q * k + c] = z[(size_t)q * nk + ix[c]];
    }
    HIP_TRY(hipMemcpyAsync(Zs, zs.data(), sizeof(double) * zs.size(), hipMemcpyHostToDevice, s));
    const long nt = (long)D * k;
    hipLaunchKernelGGL(pilot::lz_ritz_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, V, D, nk, Zs, k, (const double *)nullptr,
                       d_pcs);
    hipLaunchKernelGGL(pilot::pca_offsets_kernel, dim3(1), dim3(64), 0, s, op.sbar, d_pcs, D, k, off);
    op.scores(d_pcs, k, off, d_scores);
    hipLaunchKernelGGL(pilot::pca_sign_kernel, dim3(k), dim3(pilot::DM_RED), 0, s, d_scores, n, k, d_pcs, D);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(scores, d_scores, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pcs, d_pcs, sizeof(double) * (size_t)D * k, hipMemcpyDeviceToHost));
    info[0] = steps;
    info[1] = (converged ? 0 : PILOT_OT_PCA_NOT_CONVERGED) | (deficient ? PILOT_OT_PCA_RANK_DEFICIENT : 0);
    return PILOT_OT_OK;
}

// mean / m2 of the selected columns (host) -> mu, sigma, c on the device.  stats: 7 x D doubles = mean | m2 | mu | sigma | c | sbar | ssq
int constants(const std::vector<double> &mean, const std::vector<double> &m2, long long n, int D, int scale, int implicit, double maxv,
              double **stats) {
    HIP_TRY(pilot::ws(pilot::WS_PCA_STATS, 7 * (size_t)D, stats));
    double *st = *stats;
    HIP_TRY(hipMemcpy(st, mean.data(), sizeof(double) * D, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + D, m2.data(), sizeof(double) * D, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pilot::pca_constants_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, nullptr, st, st + D, n, D, scale, implicit,
                       maxv, st + 2 * (size_t)D, st + 3 * (size_t)D, st + 4 * (size_t)D);
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}

int upload_cols(const int *cols, int n_sel, int **d_cols) {
    *d_cols = nullptr;
    if (!cols) return PILOT_OT_OK;
    HIP_TRY(pilot::ws(pilot::WS_PCA_COLS, (size_t)n_sel, d_cols));
    HIP_TRY(hipMemcpy(*d_cols, cols, sizeof(int) * (size_t)n_sel, hipMemcpyHostToDevice));
    return PILOT_OT_OK;
}

unsigned row_blocks(long long n) { return (unsigned)((n + pilot::PCA_ROW_WAVES - 1) / pilot::PCA_ROW_WAVES); }

}  // namespace

PILOT_API int pilot_ot_csr_pca(pilot_ot_csr *c, const int *cols, int n_sel, int scale, double max_value, int n_comps, double *scores,
                               double *pcs, double *variance, double *variance_ratio, int *info) {
    if (!c || !scores || !pcs || !variance || !variance_ratio || !info) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_args(c->n, c->n_cols, cols, n_sel, scale, max_value, n_comps)) return rc;
    const long long n = c->n;
    const int D = n_sel;
    const double maxv = scale ? max_value : std::numeric_limits<double>::infinity();

    // column moments from the column form (built here if need be)
    std::vector<int> codes((size_t)n, 0);
    std::vector<double> mean((size_t)D), m2((size_t)D);
    long long count = 0;
    if (int rc = pilot_ot_csr_group_moments(c, codes.data(), 1, cols, D, 0, &count, mean.data(), m2.data())) return rc;
    if (int rc = check_finite(mean, m2)) return rc;
    double *stats;
    if (int rc = constants(mean, m2, n, D, scale, 1, maxv, &stats)) return rc;
    const double *mu = stats + 2 * (size_t)D, *sg = mu + D, *cc = sg + D;
    double *sbar = stats + 5 * (size_t)D, *d_ssq = sbar + D;

    int *d_cols, *d_pos = nullptr;
    if (int rc = upload_cols(cols, D, &d_cols)) return rc;
    if (cols) {
        std::vector<int> pos((size_t)c->n_cols, -1);
        for (int j = 0; j < D; ++j) pos[cols[j]] = j;
        HIP_TRY(pilot::ws(pilot::WS_PCA_POS, pos.size(), &d_pos));
        HIP_TRY(hipMemcpy(d_pos, pos.data(), sizeof(int) * pos.size(), hipMemcpyHostToDevice));
    }
    const size_t m = (size_t)std::max<long long>(c->nnz, 1);
    int *sidx;
    double *sval, *csval;
    HIP_TRY(pilot::ws(pilot::WS_PCA_SIDX, m, &sidx));
    HIP_TRY(pilot::ws(pilot::WS_PCA_SVAL, m, &sval));
    HIP_TRY(pilot::ws(pilot::WS_PCA_CSVAL, m, &csval));
    if (c->nnz > 0) {
        const int grid = pilot::grid_for((long)c->nnz, 256, pilot::cu_count());
        if (c->dtype == 0)
            hipLaunchKernelGGL(pilot::pca_row_values_kernel<float>, dim3(grid), dim3(256), 0, nullptr, c->indices, static_cast<const float *>(c->data),
                               c->nnz, d_pos, mu, sg, cc, maxv, sidx, sval);
        else
            hipLaunchKernelGGL(pilot::pca_row_values_kernel<double>, dim3(grid), dim3(256), 0, nullptr, c->indices,
                               static_cast<const double *>(c->data), c->nnz, d_pos, mu, sg, cc, maxv, sidx, sval);
    }
    if (c->dtype == 0)
        hipLaunchKernelGGL(pilot::pca_column_pass_kernel<float>, dim3((unsigned)D), dim3(pilot::PCA_COL_THREADS), 0, nullptr, c->colptr,
                           static_cast<const float *>(c->cdata), d_cols, n, mu, sg, cc, maxv, csval, sbar, d_ssq);
    else
        hipLaunchKernelGGL(pilot::pca_column_pass_kernel<double>, dim3((unsigned)D), dim3(pilot::PCA_COL_THREADS), 0, nullptr, c->colptr,
                           static_cast<const double *>(c->cdata), d_cols, n, mu, sg, cc, maxv, csval, sbar, d_ssq);
    HIP_TRY(hipGetLastError());
    std::vector<double> ssq((size_t)D);
    HIP_TRY(hipMemcpy(ssq.data(), d_ssq, sizeof(double) * D, hipMemcpyDeviceToHost));

    Operator op;
    op.n = n;
    op.D = D;
    op.sbar = sbar;
    op.forward = [&](const double *v, const double *dot, double *t) {
        hipLaunchKernelGGL(pilot::pca_csr_forward_kernel, dim3(row_blocks(n)), dim3(64 * pilot::PCA_ROW_WAVES), 0, nullptr, c->indptr, sidx, sval, n,
                           v, dot, t);
    };
    op.transposed = [&](const double *t, const double *part, double *w) {
        hipLaunchKernelGGL(pilot::pca_csr_transposed_kernel, dim3((unsigned)D), dim3(pilot::PCA_COL_THREADS), 0, nullptr, c->colptr, c->rowidx, csval,
                           d_cols, t, part, sbar, w);
    };
    op.scores = [&](const double *Vm, int k, const double *off, double *out) {
        hipLaunchKernelGGL(pilot::pca_csr_scores_kernel, dim3(row_blocks(n)), dim3(64 * pilot::PCA_ROW_WAVES), 0, nullptr, c->indptr, sidx, sval, n,
                           Vm, k, off, out);
    };
    return solve(op, ssq, n_comps, scores, pcs, variance, variance_ratio, info);
}

PILOT_API int pilot_ot_pca(const void *Y, int Y_is_device, int dtype, long long n, int n_cols_total, long long ld, const int *cols, int n_sel,
                           int scale, double max_value, int n_comps, double *scores, double *pcs, double *variance, double *variance_ratio,
                           int *info) {
    if (!Y || !scores || !pcs || !variance || !variance_ratio || !info) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n_cols_total < 1) return fail(PILOT_OT_EINVAL, "n_cols_total=%d", n_cols_total);
    if (int rc = pilot::check_ld(ld, n_cols_total)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (int rc = check_args(n, n_cols_total, cols, n_sel, scale, max_value, n_comps)) return rc;
    const int D = n_sel;
    const double maxv = scale ? max_value : std::numeric_limits<double>::infinity();

    std::vector<int> codes((size_t)n, 0);
    std::vector<double> mean((size_t)D), m2((size_t)D);
    long long count = 0;
    if (int rc = pilot_ot_group_moments(Y, Y_is_device, dtype, n, n_cols_total, ld, codes.data(), 1, cols, D, 0, &count, mean.data(), m2.data()))
        return rc;
    if (int rc = check_finite(mean, m2)) return rc;
    double *stats;
    if (int rc = constants(mean, m2, n, D, scale, 0, maxv, &stats)) return rc;
    const double *mu = stats + 2 * (size_t)D, *sg = mu + D;
    double *sbar = stats + 5 * (size_t)D, *d_ssq = sbar + D;
    int *d_cols;
    if (int rc = upload_cols(cols, D, &d_cols)) return rc;

    const void *y;
    long long y_ld;
    if (int rc = pilot::stage_dense(Y, Y_is_device, pilot::elem_size(dtype), n, n_cols_total, ld, pilot::WS_PCA_Y, &y, &y_ld)) return rc;
    const int n_slices = (int)((n + pilot::PCA_DENSE_SLICE - 1) / pilot::PCA_DENSE_SLICE);
    if (n_slices > 65535) return fail(PILOT_OT_ENOTSUP, "n=%lld rows: more than 65535 slices of %d rows", n, pilot::PCA_DENSE_SLICE);
    double *S, *partw;
    HIP_TRY(pilot::ws(pilot::WS_PCA_S, (size_t)n * D, &S));
    HIP_TRY(pilot::ws(pilot::WS_PCA_PARTW, (size_t)n_slices * D, &partw));
    const int grid = pilot::grid_for((long)(n * D), 256, pilot::cu_count());
    if (dtype == 0)
        hipLaunchKernelGGL(pilot::pca_dense_build_kernel<float>, dim3(grid), dim3(256), 0, nullptr, static_cast<const float *>(y), y_ld, d_cols, n, D,
                           mu, sg, maxv, S);
    else
        hipLaunchKernelGGL(pilot::pca_dense_build_kernel<double>, dim3(grid), dim3(256), 0, nullptr, static_cast<const double *>(y), y_ld, d_cols, n,
                           D, mu, sg, maxv, S);
    hipLaunchKernelGGL(pilot::pca_dense_column_pass_kernel, dim3((unsigned)D), dim3(pilot::PCA_COL_THREADS), 0, nullptr, S, n, D, sbar, d_ssq);
    HIP_TRY(hipGetLastError());
    std::vector<double> ssq((size_t)D);
    HIP_TRY(hipMemcpy(ssq.data(), d_ssq, sizeof(double) * D, hipMemcpyDeviceToHost));

    Operator op;
    op.n = n;
    op.D = D;
    op.sbar = sbar;
    op.forward = [&](const double *v, const double *dot, double *t) {
        hipLaunchKernelGGL(pilot::pca_dense_forward_kernel, dim3(row_blocks(n)), dim3(64 * pilot::PCA_ROW_WAVES), 0, nullptr, S, n, D, v, dot, t);
    };
    op.transposed = [&](const double *t, const double *part, double *w) {
        hipLaunchKernelGGL(pilot::pca_dense_transposed_kernel, dim3((unsigned)((D + 63) / 64), (unsigned)n_slices), dim3(256), 0, nullptr, S, n, D, t,
                           partw);
        hipLaunchKernelGGL(pilot::pca_dense_join_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, nullptr, partw, n_slices, D, part, sbar, w);
    };
    op.scores = [&](const double *Vm, int k, const double *off, double *out) {
        hipLaunchKernelGGL(pilot::pca_dense_scores_kernel, dim3(row_blocks(n)), dim3(64 * pilot::PCA_ROW_WAVES), 0, nullptr, S, n, D, Vm, k, off, out);
    };
    return solve(op, ssq, n_comps, scores, pcs, variance, variance_ratio, info);
}
