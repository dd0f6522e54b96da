// C ABI of the negative-binomial GLM for a one-factor design (include/pilot_ot.h, section "negative-binomial GLM"; kernels:
// nb_glm_kernels.hpp, nb_shrink_kernel.hpp, nb_rlog_kernel.hpp).  Y is a host array (copied whole, packed) or a row-major buffer in HBM with its own leading dimension;
// codes, size factors, dispersions and the results are host arrays.  The host orders the samples by group once per call.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "abi_common.hpp"
#include "nb_glm_kernels.hpp"
#include "nb_rlog_kernel.hpp"
#include "nb_shrink_kernel.hpp"

namespace {

using pilot::nb_u64;

// the samples in group order, what both kernels walk
struct Design {
    std::vector<int> order, gof, gstart;
    std::vector<double> ss;
};

// every check of (m, codes, n_groups, size_factors), then the sorted design.  No HIP call.
int make_design(long long m, const int *codes, int n_groups, const double *sf, Design &d) {
    if (m < 2) return fail(PILOT_OT_EINVAL, "m=%lld samples: at least 2", m);
    if (m > INT_MAX) return fail(PILOT_OT_ENOTSUP, "m=%lld samples need more than 32-bit indices", m);
    if (n_groups < 2 || n_groups > m - 1)
        return fail(PILOT_OT_EINVAL, "n_groups=%d must be in [2, m - 1 = %lld] (a residual degree of freedom is needed)", n_groups, m - 1);
    d.gstart.assign((size_t)n_groups + 1, 0);
    for (long long i = 0; i < m; ++i) {
        if (codes[i] < 0 || codes[i] >= n_groups) return fail(PILOT_OT_EINVAL, "codes[%lld]=%d outside [0, %d)", i, codes[i], n_groups);
        if (!(std::isfinite(sf[i]) && sf[i] > 0.0)) return fail(PILOT_OT_EINVAL, "size_factors[%lld]=%g must be positive and finite", i, sf[i]);
        ++d.gstart[(size_t)codes[i] + 1];
    }
    for (int g = 0; g < n_groups; ++g) {
        if (d.gstart[(size_t)g + 1] == 0) return fail(PILOT_OT_EINVAL, "group %d has no sample", g);
        d.gstart[(size_t)g + 1] += d.gstart[g];
    }
    std::vector<int> at(d.gstart.begin(), d.gstart.end() - 1);
    d.order.resize((size_t)m);
    d.gof.resize((size_t)m);
    d.ss.resize((size_t)m);
    for (long long i = 0; i < m; ++i) {
        const int p = at[codes[i]]++;
        d.order[p] = (int)i;
        d.gof[p] = codes[i];
        d.ss[p] = sf[i];
    }
    return PILOT_OT_OK;
}

struct DevDesign {
    int *order, *gof, *gstart;
    double *ss;
};

int upload_design(const Design &d, DevDesign &dev) {
    const size_t m = d.order.size(), k1 = d.gstart.size();
    int *ints;
    HIP_TRY(pilot::ws(pilot::WS_NB_INT, 2 * m + k1, &ints));
    HIP_TRY(pilot::ws(pilot::WS_NB_SF, m, &dev.ss));
    dev.order = ints;
    dev.gof = ints + m;
    dev.gstart = dev.gof + m;
    HIP_TRY(hipMemcpy(dev.order, d.order.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev.gof, d.gof.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev.gstart, d.gstart.data(), sizeof(int) * k1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev.ss, d.ss.data(), sizeof(double) * m, hipMemcpyHostToDevice));
    return PILOT_OT_OK;
}

// the first negative or non-finite count of Y, if any, as PILOT_OT_EINVAL
template <typename T> int check_counts(const void *y, long long ld, long long m, int n_genes, long long *bad_row, int *bad_col) {
    nb_u64 *d_bad, bad = 0;
    HIP_TRY(pilot::ws(pilot::WS_NB_BAD, 1, &d_bad));
    HIP_TRY(hipMemsetAsync(d_bad, 0xFF, sizeof(nb_u64), nullptr));
    hipLaunchKernelGGL(pilot::nb_check_kernel<T>, dim3((unsigned)pilot::grid_for((long)(m * n_genes), 256, pilot::cu_count())), dim3(256), 0,
                       nullptr, static_cast<const T *>(y), ld, m, n_genes, d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad == pilot::NB_NO_BAD) return PILOT_OT_OK;
    const int col = (int)(bad >> 32);
    const long long row = (long long)(bad & 0xFFFFFFFFull);
    if (bad_row) *bad_row = row;
    if (bad_col) *bad_col = col;
    return fail(PILOT_OT_EINVAL, "Y[%lld, %d] is negative, NaN or infinite: a count is expected (row %lld, column %d)", row, col, row, col);
}

template <typename T>
int dispersions(const void *y, long long ld, int m, int n_genes, int k, const DevDesign &dd, const double *log_prior_mean, double prior_var,
                double *log_disp, double *objective, double *fitted_mean, long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    const size_t G = (size_t)n_genes;
    double *d_out, *d_prior = nullptr;
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, 2 * G + (fitted_mean ? G * k : 0), &d_out));
    if (log_prior_mean) {
        HIP_TRY(pilot::ws(pilot::WS_NB_PRIOR, G, &d_prior));
        HIP_TRY(hipMemcpy(d_prior, log_prior_mean, sizeof(double) * G, hipMemcpyHostToDevice));
    }
    const size_t lds = sizeof(double) * (2 * (size_t)m + (size_t)k);
    auto kern = pilot::nb_dispersion_kernel<T>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)n_genes), dim3(64), lds, nullptr, static_cast<const T *>(y), ld, m, k, dd.order, dd.gof, dd.ss,
                       dd.gstart, d_prior, prior_var, d_out, d_out + G, fitted_mean ? d_out + 2 * G : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(log_disp, d_out, sizeof(double) * G, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(objective, d_out + G, sizeof(double) * G, hipMemcpyDeviceToHost));
    if (fitted_mean) HIP_TRY(hipMemcpy(fitted_mean, d_out + 2 * G, sizeof(double) * G * k, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

template <typename T>
int group_fits(const void *y, long long ld, long long m, int n_genes, int k, const DevDesign &dd, const double *dispersion, double *q, double *w,
               int *steps, int *flags) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, nullptr, nullptr)) return rc;
    const size_t G = (size_t)n_genes, n_out = G * (size_t)k;
    double *d_dbl;
    int *d_int;
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, G + 2 * n_out, &d_dbl));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, 2 * n_out, &d_int));
    HIP_TRY(hipMemcpy(d_dbl, dispersion, sizeof(double) * G, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pilot::nb_group_fit_kernel<T>, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, nullptr, static_cast<const T *>(y), ld,
                       n_genes, k, dd.order, dd.ss, dd.gstart, d_dbl, d_dbl + G, d_dbl + G + n_out, d_int, d_int + n_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(q, d_dbl + G, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(w, d_dbl + G + n_out, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(steps, d_int, sizeof(int) * n_out, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flags, d_int + n_out, sizeof(int) * n_out, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

template <typename T>
int shrink(const void *y, long long ld, int m, int n_genes, const DevDesign &dd, int n0, const double *dispersion, const double *far_end,
           double prior_scale, double intercept_scale, double *beta0, double *beta1, double *objective, double *info, int *flags,
           long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    const size_t G = (size_t)n_genes;
    double *d_dbl;                                           // dispersion, far_end | beta0, beta1, objective, info (2 a gene)
    int *d_flags;
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, 7 * G, &d_dbl));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, G, &d_flags));
    HIP_TRY(hipMemcpy(d_dbl, dispersion, sizeof(double) * G, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_dbl + G, far_end, sizeof(double) * G, hipMemcpyHostToDevice));
    const size_t lds = sizeof(double) * 2 * (size_t)m;
    auto kern = pilot::nb_shrink_kernel<T>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)n_genes), dim3(64), lds, nullptr, static_cast<const T *>(y), ld, m, n0, dd.order, dd.ss, d_dbl,
                       d_dbl + G, prior_scale, intercept_scale, d_dbl + 2 * G, d_dbl + 3 * G, d_dbl + 4 * G, d_dbl + 5 * G, d_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(beta0, d_dbl + 2 * G, sizeof(double) * G, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(beta1, d_dbl + 3 * G, sizeof(double) * G, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(objective, d_dbl + 4 * G, sizeof(double) * G, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(info, d_dbl + 5 * G, sizeof(double) * 2 * G, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flags, d_flags, sizeof(int) * G, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

// every check of (m, size_factors) of the calls without groups.  No HIP call.
int check_samples(long long m, const double *sf) {
    if (m < 2) return fail(PILOT_OT_EINVAL, "m=%lld samples: at least 2", m);
    if (m > INT_MAX) return fail(PILOT_OT_ENOTSUP, "m=%lld samples need more than 32-bit indices", m);
    for (long long i = 0; i < m; ++i)
        if (!(std::isfinite(sf[i]) && sf[i] > 0.0)) return fail(PILOT_OT_EINVAL, "size_factors[%lld]=%g must be positive and finite", i, sf[i]);
    return PILOT_OT_OK;
}

// the design `~ 1` of m samples (blind): one group, the samples in their own order
int make_blind_design(long long m, const double *sf, Design &d) {
    if (int rc = check_samples(m, sf)) return rc;
    d.order.resize((size_t)m);
    for (long long i = 0; i < m; ++i) d.order[(size_t)i] = (int)i;
    d.gof.assign((size_t)m, 0);
    d.gstart = {0, (int)m};
    d.ss.assign(sf, sf + m);
    return PILOT_OT_OK;
}

template <typename T>
int rlog(const void *y, long long ld, int m, int n_genes, const double *sf, const double *dispersion, double prior_var, void *out,
         int out_is_device, long long ld_out, double *intercept, int *steps, int *flags, long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    const size_t G = (size_t)n_genes, M = (size_t)m;
    std::vector<double> s(2 * M);                            // the size factors, then their logarithms
    for (size_t j = 0; j < M; ++j) { s[j] = sf[j]; s[M + j] = std::log(sf[j]); }
    double *d_sf, *d_disp, *d_dbl;                           // d_dbl: intercept | the packed m x G result when `out` is on the host
    int *d_int;                                              // steps, flags
    HIP_TRY(pilot::ws(pilot::WS_NB_SF, 2 * M, &d_sf));
    HIP_TRY(pilot::ws(pilot::WS_NB_PRIOR, G, &d_disp));
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, G + (out_is_device ? 0 : M * G), &d_dbl));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, 2 * G, &d_int));
    HIP_TRY(hipMemcpy(d_sf, s.data(), sizeof(double) * 2 * M, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_disp, dispersion, sizeof(double) * G, hipMemcpyHostToDevice));
    double *d_res = out_is_device ? static_cast<double *>(out) : d_dbl + G;
    const long long ld_res = out_is_device ? ld_out : (long long)n_genes;
    const double ln2 = pilot::NB_RLOG_LN2, lambda = ln2 * ln2 / prior_var, lambda0 = pilot::NB_RLOG_INTERCEPT_RIDGE * ln2 * ln2;
    const size_t lds = sizeof(double) * 3 * M;
    auto kern = pilot::nb_rlog_kernel<T>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)n_genes), dim3(64), lds, nullptr, static_cast<const T *>(y), ld, m, d_sf, d_disp, lambda, lambda0,
                       d_res, ld_res, d_dbl, d_int, d_int + G);
    HIP_TRY(hipGetLastError());
    if (!out_is_device)
        HIP_TRY(hipMemcpy2D(out, sizeof(double) * (size_t)ld_out, d_res, sizeof(double) * G, sizeof(double) * G, M, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(intercept, d_dbl, sizeof(double) * G, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(steps, d_int, sizeof(int) * G, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flags, d_int + G, sizeof(int) * G, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

// a dispersion is NaN (the gene is left out) or within [minDisp, maxDisp]
int check_dispersions(const double *dispersion, int n_genes, long long m) {
    const double max_disp = pilot::nb_max_disp(m);
    for (int j = 0; j < n_genes; ++j)
        if (!std::isnan(dispersion[j]) && !(dispersion[j] >= pilot::NB_MIN_DISP && dispersion[j] <= max_disp))
            return fail(PILOT_OT_EINVAL, "dispersion[%d]=%g outside [%g, %g] (NaN: the gene is left out)", j, dispersion[j], pilot::NB_MIN_DISP,
                        max_disp);
    return PILOT_OT_OK;
}

int check_matrix(int dtype, int n_genes, long long ld) {
    if (n_genes < 1) return fail(PILOT_OT_EINVAL, "n_genes=%d", n_genes);
    if (int rc = pilot::check_ld(ld, n_genes)) return rc;
    return pilot::check_dtype(dtype);
}

}  // namespace

PILOT_API int pilot_ot_nb_glm_max_samples(void) { return pilot::NB_MAX_SAMPLES; }

PILOT_API int pilot_ot_nb_dispersions(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                                      int n_groups, const double *size_factors, const double *log_prior_mean, double prior_var,
                                      double *log_disp, double *objective, double *fitted_mean, long long *bad_row, int *bad_col) {
    if (bad_row) *bad_row = -1;
    if (bad_col) *bad_col = -1;
    if (!Y || !codes || !size_factors || !log_disp || !objective) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_matrix(dtype, n_genes, ld)) return rc;
    if (log_prior_mean && !(std::isfinite(prior_var) && prior_var > 0.0))
        return fail(PILOT_OT_EINVAL, "prior_var=%g must be positive and finite when a prior is given", prior_var);
    Design d;
    if (int rc = make_design(m, codes, n_groups, size_factors, d)) return rc;
    if (m > pilot::NB_MAX_SAMPLES)
        return fail(PILOT_OT_ENOTSUP, "m=%lld samples: a gene's counts and fitted means are staged in LDS, at most %d", m, pilot::NB_MAX_SAMPLES);
    const void *y;
    long long y_ld;
    if (int rc = pilot::stage_dense(Y, Y_is_device, pilot::elem_size(dtype), m, n_genes, ld, pilot::WS_NB_Y, &y, &y_ld)) return rc;
    DevDesign dd;
    if (int rc = upload_design(d, dd)) return rc;
    return dtype == 0 ? dispersions<float>(y, y_ld, (int)m, n_genes, n_groups, dd, log_prior_mean, prior_var, log_disp, objective, fitted_mean,
                                           bad_row, bad_col)
                      : dispersions<double>(y, y_ld, (int)m, n_genes, n_groups, dd, log_prior_mean, prior_var, log_disp, objective, fitted_mean,
                                            bad_row, bad_col);
}

PILOT_API int pilot_ot_nb_dispersions_blind(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld,
                                            const double *size_factors, double *log_disp, double *objective, double *base_mean,
                                            long long *bad_row, int *bad_col) {
    if (bad_row) *bad_row = -1;
    if (bad_col) *bad_col = -1;
    if (!Y || !size_factors || !log_disp || !objective) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_matrix(dtype, n_genes, ld)) return rc;
    Design d;
    if (int rc = make_blind_design(m, size_factors, d)) return rc;
    if (m > pilot::NB_MAX_SAMPLES)
        return fail(PILOT_OT_ENOTSUP, "m=%lld samples: a gene's counts and fitted means are staged in LDS, at most %d", m, pilot::NB_MAX_SAMPLES);
    const void *y;
    long long y_ld;
    if (int rc = pilot::stage_dense(Y, Y_is_device, pilot::elem_size(dtype), m, n_genes, ld, pilot::WS_NB_Y, &y, &y_ld)) return rc;
    DevDesign dd;
    if (int rc = upload_design(d, dd)) return rc;
    return dtype == 0 ? dispersions<float>(y, y_ld, (int)m, n_genes, 1, dd, nullptr, 0.0, log_disp, objective, base_mean, bad_row, bad_col)
                      : dispersions<double>(y, y_ld, (int)m, n_genes, 1, dd, nullptr, 0.0, log_disp, objective, base_mean, bad_row, bad_col);
}

PILOT_API int pilot_ot_nb_group_fits(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                                     int n_groups, const double *size_factors, const double *dispersion, double *q, double *w, int *steps,
                                     int *flags, int *n_not_converged) {
    if (n_not_converged) *n_not_converged = 0;
    if (!Y || !codes || !size_factors || !dispersion || !q || !w || !steps || !flags) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_matrix(dtype, n_genes, ld)) return rc;
    Design d;
    if (int rc = make_design(m, codes, n_groups, size_factors, d)) return rc;
    if (int rc = check_dispersions(dispersion, n_genes, m)) return rc;
    if ((long long)n_genes * n_groups > INT_MAX)
        return fail(PILOT_OT_ENOTSUP, "n_genes * n_groups = %lld results need more than 32-bit indices", (long long)n_genes * n_groups);
    const void *y;
    long long y_ld;
    if (int rc = pilot::stage_dense(Y, Y_is_device, pilot::elem_size(dtype), m, n_genes, ld, pilot::WS_NB_Y, &y, &y_ld)) return rc;
    DevDesign dd;
    if (int rc = upload_design(d, dd)) return rc;
    if (int rc = dtype == 0 ? group_fits<float>(y, y_ld, m, n_genes, n_groups, dd, dispersion, q, w, steps, flags)
                            : group_fits<double>(y, y_ld, m, n_genes, n_groups, dd, dispersion, q, w, steps, flags))
        return rc;
    int bad = 0;
    for (long long t = 0; t < (long long)n_genes * n_groups; ++t) bad += (flags[t] & pilot::NB_FLAG_NOT_CONVERGED) != 0;
    if (n_not_converged) *n_not_converged = bad;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_nb_shrink(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                                 const double *size_factors, const double *dispersion, const double *far_end, double prior_scale,
                                 double intercept_scale, double *beta0, double *beta1, double *objective, double *info, int *flags,
                                 int *n_at_bound, long long *bad_row, int *bad_col) {
    if (bad_row) *bad_row = -1;
    if (bad_col) *bad_col = -1;
    if (n_at_bound) *n_at_bound = 0;
    if (!Y || !codes || !size_factors || !dispersion || !far_end || !beta0 || !beta1 || !objective || !info || !flags)
        return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_matrix(dtype, n_genes, ld)) return rc;
    if (!(std::isfinite(prior_scale) && prior_scale > 0.0)) return fail(PILOT_OT_EINVAL, "prior_scale=%g must be positive and finite", prior_scale);
    if (!(std::isfinite(intercept_scale) && intercept_scale > 0.0))
        return fail(PILOT_OT_EINVAL, "intercept_scale=%g must be positive and finite", intercept_scale);
    Design d;
    if (int rc = make_design(m, codes, 2, size_factors, d)) return rc;
    if (int rc = check_dispersions(dispersion, n_genes, m)) return rc;
    for (int j = 0; j < n_genes; ++j)
        if (!std::isfinite(far_end[j])) return fail(PILOT_OT_EINVAL, "far_end[%d]=%g must be finite", j, far_end[j]);
    if (m > pilot::NB_MAX_SAMPLES)
        return fail(PILOT_OT_ENOTSUP, "m=%lld samples: a gene's counts and size factors are staged in LDS, at most %d", m, pilot::NB_MAX_SAMPLES);
    const void *y;
    long long y_ld;
    if (int rc = pilot::stage_dense(Y, Y_is_device, pilot::elem_size(dtype), m, n_genes, ld, pilot::WS_NB_Y, &y, &y_ld)) return rc;
    DevDesign dd;
    if (int rc = upload_design(d, dd)) return rc;
    if (int rc = dtype == 0 ? shrink<float>(y, y_ld, (int)m, n_genes, dd, d.gstart[1], dispersion, far_end, prior_scale, intercept_scale, beta0,
                                            beta1, objective, info, flags, bad_row, bad_col)
                            : shrink<double>(y, y_ld, (int)m, n_genes, dd, d.gstart[1], dispersion, far_end, prior_scale, intercept_scale, beta0,
                                             beta1, objective, info, flags, bad_row, bad_col))
        return rc;
    int at_bound = 0;
    for (int j = 0; j < n_genes; ++j) at_bound += (flags[j] & pilot::NB_FLAG_AT_BOUND) != 0;
    if (n_at_bound) *n_at_bound = at_bound;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_nb_rlog(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *size_factors,
                               const double *dispersion, double prior_var, void *out, int out_is_device, long long ld_out,
                               double *intercept, int *steps, int *flags, int *n_not_converged, long long *bad_row, int *bad_col) {
    if (bad_row) *bad_row = -1;
    if (bad_col) *bad_col = -1;
    if (n_not_converged) *n_not_converged = 0;
    if (!Y || !size_factors || !dispersion || !out || !intercept || !steps || !flags) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_matrix(dtype, n_genes, ld)) return rc;
    if (ld_out < n_genes) return fail(PILOT_OT_EINVAL, "ld_out=%lld is smaller than n_genes=%d", ld_out, n_genes);
    if (int rc = check_samples(m, size_factors)) return rc;
    if (!(std::isfinite(prior_var) && prior_var > 0.0)) return fail(PILOT_OT_EINVAL, "prior_var=%g must be positive and finite", prior_var);
    if (int rc = check_dispersions(dispersion, n_genes, m)) return rc;
    if (m > pilot::NB_MAX_SAMPLES)
        return fail(PILOT_OT_ENOTSUP, "m=%lld samples: a gene's counts, log size factors and coefficients are staged in LDS, at most %d", m,
                    pilot::NB_MAX_SAMPLES);
    const void *y;
    long long y_ld;
    if (int rc = pilot::stage_dense(Y, Y_is_device, pilot::elem_size(dtype), m, n_genes, ld, pilot::WS_NB_Y, &y, &y_ld)) return rc;
    if (int rc = dtype == 0 ? rlog<float>(y, y_ld, (int)m, n_genes, size_factors, dispersion, prior_var, out, out_is_device, ld_out, intercept,
                                          steps, flags, bad_row, bad_col)
                            : rlog<double>(y, y_ld, (int)m, n_genes, size_factors, dispersion, prior_var, out, out_is_device, ld_out, intercept,
                                           steps, flags, bad_row, bad_col))
        return rc;
    int bad = 0;
    for (int j = 0; j < n_genes; ++j) bad += (flags[j] & pilot::NB_FLAG_NOT_CONVERGED) != 0;
    if (n_not_converged) *n_not_converged = bad;
    return PILOT_OT_OK;
}
