// C ABI of the negative-binomial GLM for a one-factor design and, at the end, for a general one (include/pilot_ot.h, section
// "negative-binomial GLM"; kernels: nb_glm_kernels.hpp, nb_shrink_kernel.hpp, nb_rlog_kernel.hpp, nb_cooks_kernel.hpp, nb_design_kernels.hpp,
// nb_design_shrink_kernel.hpp, nb_design_cooks_kernel.hpp).  Y is a host array (copied whole, packed) or a row-major buffer in HBM with its own leading dimension;
// codes, size factors, dispersions and the results are host arrays.  The host orders the samples by group once per call.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "abi_common.hpp"
#include "nb_cooks_kernel.hpp"
#include "nb_design_cooks_kernel.hpp"
#include "nb_design_kernels.hpp"
#include "nb_design_shrink_kernel.hpp"
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

// every check of (m, size_factors) and, with codes (a grouped call), of (n_groups, codes), in the order the calls have always
// refused them.  No HIP call.
int check_samples(long long m, const double *sf, const int *codes = nullptr, int n_groups = 1) {
    if (m < 2) return fail(PILOT_OT_EINVAL, "m=%lld samples: at least 2", m);
    if (m > INT_MAX) return fail(PILOT_OT_ENOTSUP, "m=%lld samples need more than 32-bit indices", m);
    if (codes && (n_groups < 2 || n_groups > m - 1))
        return fail(PILOT_OT_EINVAL, "n_groups=%d must be in [2, m - 1 = %lld] (a residual degree of freedom is needed)", n_groups, m - 1);
    for (long long i = 0; i < m; ++i) {
        if (codes && (codes[i] < 0 || codes[i] >= n_groups)) return fail(PILOT_OT_EINVAL, "codes[%lld]=%d outside [0, %d)", i, codes[i], n_groups);
        if (!(std::isfinite(sf[i]) && sf[i] > 0.0)) return fail(PILOT_OT_EINVAL, "size_factors[%lld]=%g must be positive and finite", i, sf[i]);
    }
    return PILOT_OT_OK;
}

// the samples ordered by their code (every one of [0, n_groups), checked by the caller; NULL: all 0), `what` names a code in a refusal
int sort_samples(long long m, const int *codes, int n_groups, const double *sf, const char *what, Design &d) {
    const auto code = [codes](long long i) { return codes ? codes[i] : 0; };
    d.gstart.assign((size_t)n_groups + 1, 0);
    for (long long i = 0; i < m; ++i) ++d.gstart[(size_t)code(i) + 1];
    for (int g = 0; g < n_groups; ++g) {
        if (d.gstart[(size_t)g + 1] == 0) return fail(PILOT_OT_EINVAL, "%s %d has no sample", what, g);
        d.gstart[(size_t)g + 1] += d.gstart[g];
    }
    std::vector<int> at(d.gstart.begin(), d.gstart.end() - 1);
    d.order.resize((size_t)m);
    d.gof.resize((size_t)m);
    d.ss.resize((size_t)m);
    for (long long i = 0; i < m; ++i) {
        const int p = at[code(i)]++;
        d.order[p] = (int)i;
        d.gof[p] = code(i);
        d.ss[p] = sf[i];
    }
    return PILOT_OT_OK;
}

// check_samples, then the sorted design.  Without codes: the design `~ 1` of m samples (blind), one group (n_groups = 1), the
// samples in their own order.
int make_design(long long m, const int *codes, int n_groups, const double *sf, Design &d) {
    if (int rc = check_samples(m, sf, codes, n_groups)) return rc;
    return sort_samples(m, codes, n_groups, sf, "group", d);
}

struct DevDesign {
    int *order, *gof, *gstart;
    double *ss;
};

// order, gof and gstart of the sorted samples
int upload_order(const Design &d, DevDesign &dev) {
    const size_t m = d.order.size(), k1 = d.gstart.size();
    int *ints;
    HIP_TRY(pilot::ws(pilot::WS_NB_INT, 2 * m + k1, &ints));
    dev.order = ints;
    dev.gof = ints + m;
    dev.gstart = dev.gof + m;
    HIP_TRY(hipMemcpy(dev.order, d.order.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev.gof, d.gof.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev.gstart, d.gstart.data(), sizeof(int) * k1, hipMemcpyHostToDevice));
    return PILOT_OT_OK;
}

int upload_design(const Design &d, DevDesign &dev) {
    const size_t m = d.order.size();
    if (int rc = upload_order(d, dev)) return rc;
    HIP_TRY(pilot::ws(pilot::WS_NB_SF, m, &dev.ss));
    HIP_TRY(hipMemcpy(dev.ss, d.ss.data(), sizeof(double) * m, hipMemcpyHostToDevice));
    return PILOT_OT_OK;
}

// one workgroup of one wave per gene with `lds_doubles` doubles of dynamic LDS, which the kernel is allowed first
template <typename... P, typename... A> int launch_wave_per_gene(void (*kern)(P...), int n_genes, size_t lds_doubles, A... args) {
    const size_t lds = sizeof(double) * lds_doubles;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)n_genes), dim3(64), lds, nullptr, args...);
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}

// n elements from HBM to the host
template <typename T> hipError_t fetch(T *dst, const T *src, size_t n) { return hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost); }

// An m x G float64 result the caller takes in HBM (its buffer, its leading dimension) or on the host.  For the host the kernel
// writes it packed behind the call's other doubles in the WS_NB_OUT slot -- the call asks for tail() more and says where with
// place() -- and fetch() copies it out.  out == NULL: the call returns no such matrix.
struct ResultMatrix {
    void *out;
    int on_device;
    long long ld_out;
    size_t m, G;
    double *dev = nullptr;                                   // where the kernel writes, with the leading dimension ld()
    bool staged() const { return out && !on_device; }
    size_t tail() const { return staged() ? m * G : 0; }
    long long ld() const { return on_device ? ld_out : (long long)G; }
    void place(double *slot_tail) { dev = staged() ? slot_tail : static_cast<double *>(out); }
    hipError_t fetch() const {
        if (!staged()) return hipSuccess;
        return hipMemcpy2D(out, sizeof(double) * (size_t)ld_out, dev, sizeof(double) * G, sizeof(double) * G, m, hipMemcpyDeviceToHost);
    }
};

// the first negative or non-finite count of Y, if any, as PILOT_OT_EINVAL
template <typename T> int check_counts(const void *y, long long ld, long long m, int n_genes, long long *bad_row, int *bad_col) {
    nb_u64 *d_bad, bad = 0;
    HIP_TRY(pilot::ws(pilot::WS_NB_BAD, 1, &d_bad));
    HIP_TRY(hipMemsetAsync(d_bad, 0xFF, sizeof(nb_u64), nullptr));
    hipLaunchKernelGGL(pilot::nb_check_kernel<T>, dim3((unsigned)pilot::grid_for((long)(m * n_genes), 256, pilot::cu_count())), dim3(256), 0,
                       nullptr, static_cast<const T *>(y), ld, m, n_genes, d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(fetch(&bad, d_bad, 1));
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
    if (int rc = launch_wave_per_gene(pilot::nb_dispersion_kernel<T>, n_genes, 2 * (size_t)m + (size_t)k, static_cast<const T *>(y), ld, m, k,
                                      dd.order, dd.gof, dd.ss, dd.gstart, d_prior, prior_var, d_out, d_out + G,
                                      fitted_mean ? d_out + 2 * G : nullptr))
        return rc;
    HIP_TRY(fetch(log_disp, d_out, G));
    HIP_TRY(fetch(objective, d_out + G, G));
    if (fitted_mean) HIP_TRY(fetch(fitted_mean, d_out + 2 * G, G * k));
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
    HIP_TRY(fetch(q, d_dbl + G, n_out));
    HIP_TRY(fetch(w, d_dbl + G + n_out, n_out));
    HIP_TRY(fetch(steps, d_int, n_out));
    HIP_TRY(fetch(flags, d_int + n_out, n_out));
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
    if (int rc = launch_wave_per_gene(pilot::nb_shrink_kernel<T>, n_genes, 2 * (size_t)m, static_cast<const T *>(y), ld, m, n0, dd.order, dd.ss,
                                      d_dbl, d_dbl + G, prior_scale, intercept_scale, d_dbl + 2 * G, d_dbl + 3 * G, d_dbl + 4 * G, d_dbl + 5 * G,
                                      d_flags))
        return rc;
    HIP_TRY(fetch(beta0, d_dbl + 2 * G, G));
    HIP_TRY(fetch(beta1, d_dbl + 3 * G, G));
    HIP_TRY(fetch(objective, d_dbl + 4 * G, G));
    HIP_TRY(fetch(info, d_dbl + 5 * G, 2 * G));
    HIP_TRY(fetch(flags, d_flags, G));
    return PILOT_OT_OK;
}

template <typename T>
int rlog(const void *y, long long ld, int m, int n_genes, const double *sf, const double *dispersion, double prior_var, ResultMatrix res,
         double *intercept, int *steps, int *flags, long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    const size_t G = (size_t)n_genes, M = (size_t)m;
    std::vector<double> s(2 * M);                            // the size factors, then their logarithms
    for (size_t j = 0; j < M; ++j) { s[j] = sf[j]; s[M + j] = std::log(sf[j]); }
    double *d_sf, *d_disp, *d_dbl;                           // d_dbl: intercept | the packed m x G result when `out` is on the host
    int *d_int;                                              // steps, flags
    HIP_TRY(pilot::ws(pilot::WS_NB_SF, 2 * M, &d_sf));
    HIP_TRY(pilot::ws(pilot::WS_NB_PRIOR, G, &d_disp));
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, G + res.tail(), &d_dbl));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, 2 * G, &d_int));
    HIP_TRY(hipMemcpy(d_sf, s.data(), sizeof(double) * 2 * M, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_disp, dispersion, sizeof(double) * G, hipMemcpyHostToDevice));
    res.place(d_dbl + G);
    const double ln2 = pilot::NB_RLOG_LN2, lambda = ln2 * ln2 / prior_var, lambda0 = pilot::NB_RLOG_INTERCEPT_RIDGE * ln2 * ln2;
    if (int rc = launch_wave_per_gene(pilot::nb_rlog_kernel<T>, n_genes, 3 * M, static_cast<const T *>(y), ld, m, d_sf, d_disp, lambda, lambda0,
                                      res.dev, res.ld(), d_dbl, d_int, d_int + G))
        return rc;
    HIP_TRY(res.fetch());
    HIP_TRY(fetch(intercept, d_dbl, G));
    HIP_TRY(fetch(steps, d_int, G));
    HIP_TRY(fetch(flags, d_int + G, G));
    return PILOT_OT_OK;
}

template <typename T>
int cooks(const void *y, long long ld, int m, int n_genes, int k, const DevDesign &dd, const double *dispersion, const double *q, double cutoff,
          int min_replace, double *alpha_robust, double *max_cooks, int *arg_max, int *n_above, int *n_replace, double *trimmed_base,
          ResultMatrix D, long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    const size_t G = (size_t)n_genes, M = (size_t)m, n_q = G * (size_t)k;
    size_t P = 1;                                            // the sort buffer: the power of two >= m
    while (P < M) P <<= 1;
    double *d_in, *d_out;                                    // dispersion | q;  the three double results | packed D for a host D
    int *d_int;
    HIP_TRY(pilot::ws(pilot::WS_NB_PRIOR, G + n_q, &d_in));
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, 3 * G + D.tail(), &d_out));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, 3 * G, &d_int));
    HIP_TRY(hipMemcpy(d_in, dispersion, sizeof(double) * G, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_in + G, q, sizeof(double) * n_q, hipMemcpyHostToDevice));
    D.place(d_out + 3 * G);
    if (int rc = launch_wave_per_gene(pilot::nb_cooks_kernel<T>, n_genes, 2 * M + P, static_cast<const T *>(y), ld, m, k, dd.order, dd.gof, dd.ss,
                                      dd.gstart, d_in, d_in + G, cutoff, min_replace, n_genes, d_out, d_int, D.dev, D.ld()))
        return rc;
    HIP_TRY(fetch(alpha_robust, d_out, G));
    HIP_TRY(fetch(max_cooks, d_out + G, G));
    HIP_TRY(fetch(trimmed_base, d_out + 2 * G, G));
    HIP_TRY(fetch(arg_max, d_int, G));
    HIP_TRY(fetch(n_above, d_int + G, G));
    HIP_TRY(fetch(n_replace, d_int + 2 * G, G));
    HIP_TRY(D.fetch());
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

int positive_finite(const char *name, double v, const char *when = "") {
    return std::isfinite(v) && v > 0.0 ? PILOT_OT_OK : fail(PILOT_OT_EINVAL, "%s=%g must be positive and finite%s", name, v, when);
}

int no_check() { return PILOT_OT_OK; }

// what an entry point hands the prologue, and what it gets back
struct Call {
    const void *Y;
    int Y_is_device, dtype;
    long long m;
    int n_genes;
    long long ld;
    const double *sf;
    bool design;                  // false (rlog): the samples are checked, nothing is sorted or uploaded
    const int *codes;             // of a design: NULL for `~ 1` (blind), one group
    int n_groups;
    const double *dispersion;     // nullable: checked right after the design
    const char *staged;           // nullable: what of a gene the kernel stages in LDS, so that m is limited
    const void *y;                // out: Y on the device and its leading dimension, the design on the host and the device
    long long y_ld;
    Design d;
    DevDesign dd;
};

// The one way into the five entry points: -1 into bad_row / bad_col, then every refusal in the order the calls have always made
// them -- a NULL argument, the matrix, the call's own checks `before` the design, the design (or the samples alone), the
// dispersions, the call's own checks `after` them, the LDS limit on m -- then Y staged and the design uploaded.
template <typename Before, typename After>
int prologue(Call &c, bool null_arg, long long *bad_row, int *bad_col, Before before, After after) {
    if (bad_row) *bad_row = -1;
    if (bad_col) *bad_col = -1;
    if (null_arg) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_matrix(c.dtype, c.n_genes, c.ld)) return rc;
    if (int rc = before()) return rc;
    if (int rc = c.design ? make_design(c.m, c.codes, c.n_groups, c.sf, c.d) : check_samples(c.m, c.sf)) return rc;
    if (c.dispersion)
        if (int rc = check_dispersions(c.dispersion, c.n_genes, c.m)) return rc;
    if (int rc = after()) return rc;
    if (c.staged && c.m > pilot::NB_MAX_SAMPLES)
        return fail(PILOT_OT_ENOTSUP, "m=%lld samples: a gene's %s are staged in LDS, at most %d", c.m, c.staged, pilot::NB_MAX_SAMPLES);
    if (int rc = pilot::stage_dense(c.Y, c.Y_is_device, pilot::elem_size(c.dtype), c.m, c.n_genes, c.ld, pilot::WS_NB_Y, &c.y, &c.y_ld)) return rc;
    return c.design ? upload_design(c.d, c.dd) : PILOT_OT_OK;
}

// body(T()) with T the element type of dtype code `dtype` (checked)
template <typename Body> int by_dtype(int dtype, Body body) { return dtype == 0 ? body(float()) : body(double()); }

// how many of n flag words carry `flag`, into the nullable *out
void count_flag(const int *flags, long long n, int flag, int *out) {
    int count = 0;
    for (long long t = 0; t < n; ++t) count += (flags[t] & flag) != 0;
    if (out) *out = count;
}

// pilot_ot_nb_dispersions and, without codes, pilot_ot_nb_dispersions_blind
int nb_dispersions(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes, int n_groups,
                   const double *size_factors, const double *log_prior_mean, double prior_var, double *log_disp, double *objective,
                   double *fitted_mean, long long *bad_row, int *bad_col, bool blind) {
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, true, codes, n_groups, nullptr, "counts and fitted means"};
    if (int rc = prologue(c, !Y || (!blind && !codes) || !size_factors || !log_disp || !objective, bad_row, bad_col,
                          [&] { return log_prior_mean ? positive_finite("prior_var", prior_var, " when a prior is given") : PILOT_OT_OK; }, no_check))
        return rc;
    return by_dtype(dtype, [&](auto t) {
        return dispersions<decltype(t)>(c.y, c.y_ld, (int)m, n_genes, n_groups, c.dd, log_prior_mean, prior_var, log_disp, objective, fitted_mean,
                                        bad_row, bad_col);
    });
}

}  // namespace

PILOT_API int pilot_ot_nb_glm_max_samples(void) { return pilot::NB_MAX_SAMPLES; }

PILOT_API int pilot_ot_nb_dispersions(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                                      int n_groups, const double *size_factors, const double *log_prior_mean, double prior_var,
                                      double *log_disp, double *objective, double *fitted_mean, long long *bad_row, int *bad_col) {
    return nb_dispersions(Y, Y_is_device, dtype, m, n_genes, ld, codes, n_groups, size_factors, log_prior_mean, prior_var, log_disp, objective,
                          fitted_mean, bad_row, bad_col, false);
}

PILOT_API int pilot_ot_nb_dispersions_blind(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld,
                                            const double *size_factors, double *log_disp, double *objective, double *base_mean,
                                            long long *bad_row, int *bad_col) {
    return nb_dispersions(Y, Y_is_device, dtype, m, n_genes, ld, nullptr, 1, size_factors, nullptr, 0.0, log_disp, objective, base_mean, bad_row,
                          bad_col, true);
}

PILOT_API int pilot_ot_nb_group_fits(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                                     int n_groups, const double *size_factors, const double *dispersion, double *q, double *w, int *steps,
                                     int *flags, int *n_not_converged) {
    if (n_not_converged) *n_not_converged = 0;
    const long long n_out = (long long)n_genes * n_groups;
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, true, codes, n_groups, dispersion, nullptr};
    if (int rc = prologue(c, !Y || !codes || !size_factors || !dispersion || !q || !w || !steps || !flags, nullptr, nullptr, no_check, [&] {
            return n_out > INT_MAX ? fail(PILOT_OT_ENOTSUP, "n_genes * n_groups = %lld results need more than 32-bit indices", n_out) : PILOT_OT_OK;
        }))
        return rc;
    if (int rc = by_dtype(dtype, [&](auto t) {
            return group_fits<decltype(t)>(c.y, c.y_ld, m, n_genes, n_groups, c.dd, dispersion, q, w, steps, flags);
        }))
        return rc;
    count_flag(flags, n_out, pilot::NB_FLAG_NOT_CONVERGED, n_not_converged);
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_nb_shrink(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                                 const double *size_factors, const double *dispersion, const double *far_end, double prior_scale,
                                 double intercept_scale, double *beta0, double *beta1, double *objective, double *info, int *flags,
                                 int *n_at_bound, long long *bad_row, int *bad_col) {
    if (n_at_bound) *n_at_bound = 0;
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, true, codes, 2, dispersion, "counts and size factors"};
    if (int rc = prologue(
            c, !Y || !codes || !size_factors || !dispersion || !far_end || !beta0 || !beta1 || !objective || !info || !flags, bad_row, bad_col,
            [&] {
                if (int rc = positive_finite("prior_scale", prior_scale)) return rc;
                return positive_finite("intercept_scale", intercept_scale);
            },
            [&] {
                for (int j = 0; j < n_genes; ++j)
                    if (!std::isfinite(far_end[j])) return fail(PILOT_OT_EINVAL, "far_end[%d]=%g must be finite", j, far_end[j]);
                return PILOT_OT_OK;
            }))
        return rc;
    if (int rc = by_dtype(dtype, [&](auto t) {
            return shrink<decltype(t)>(c.y, c.y_ld, (int)m, n_genes, c.dd, c.d.gstart[1], dispersion, far_end, prior_scale, intercept_scale, beta0,
                                       beta1, objective, info, flags, bad_row, bad_col);
        }))
        return rc;
    count_flag(flags, n_genes, pilot::NB_FLAG_AT_BOUND, n_at_bound);
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_nb_rlog(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *size_factors,
                               const double *dispersion, double prior_var, void *out, int out_is_device, long long ld_out,
                               double *intercept, int *steps, int *flags, int *n_not_converged, long long *bad_row, int *bad_col) {
    if (n_not_converged) *n_not_converged = 0;
    // (the prologue gets no dispersions: this call has always refused a bad prior_var after the samples and before the dispersions)
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, false, nullptr, 1, nullptr, "counts, log size factors and coefficients"};
    if (int rc = prologue(
            c, !Y || !size_factors || !dispersion || !out || !intercept || !steps || !flags, bad_row, bad_col,
            [&] { return ld_out < n_genes ? fail(PILOT_OT_EINVAL, "ld_out=%lld is smaller than n_genes=%d", ld_out, n_genes) : PILOT_OT_OK; },
            [&] {
                if (int rc = positive_finite("prior_var", prior_var)) return rc;
                return check_dispersions(dispersion, n_genes, m);
            }))
        return rc;
    if (int rc = by_dtype(dtype, [&](auto t) {
            return rlog<decltype(t)>(c.y, c.y_ld, (int)m, n_genes, size_factors, dispersion, prior_var,
                                     ResultMatrix{out, out_is_device, ld_out, (size_t)m, (size_t)n_genes}, intercept, steps, flags, bad_row, bad_col);
        }))
        return rc;
    count_flag(flags, n_genes, pilot::NB_FLAG_NOT_CONVERGED, n_not_converged);
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_nb_cooks(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes, int n_groups,
                                const double *size_factors, const double *dispersion, const double *q, double cutoff, int min_replace,
                                double *alpha_robust, double *max_cooks, int *arg_max, int *n_above, int *n_replace, double *trimmed_base,
                                void *D, int D_is_device, long long ld_D, long long *bad_row, int *bad_col) {
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, true, codes, n_groups, dispersion, "counts, normalised counts and sort buffer"};
    if (int rc = prologue(
            c, !Y || !codes || !size_factors || !dispersion || !q || !alpha_robust || !max_cooks || !arg_max || !n_above || !n_replace ||
                   !trimmed_base,
            bad_row, bad_col,
            [&] {
                if (int rc = positive_finite("cutoff", cutoff)) return rc;
                if (min_replace < pilot::NB_COOKS_MIN_GROUP)
                    return fail(PILOT_OT_EINVAL, "min_replace=%d: at least %d (smaller groups have no Cook's distance to compare)", min_replace,
                                pilot::NB_COOKS_MIN_GROUP);
                return D && ld_D < n_genes ? fail(PILOT_OT_EINVAL, "ld_D=%lld is smaller than n_genes=%d", ld_D, n_genes) : PILOT_OT_OK;
            },
            [&] {
                for (int j = 0; j < n_genes; ++j) {
                    if (std::isnan(dispersion[j])) continue;
                    for (int g = 0; g < n_groups; ++g) {
                        const double v = q[(long long)j * n_groups + g];
                        if (!(std::isfinite(v) && v > 0.0))
                            return fail(PILOT_OT_EINVAL, "q[%d, %d]=%g must be positive and finite where the gene has a dispersion", j, g, v);
                    }
                }
                return PILOT_OT_OK;
            }))
        return rc;
    return by_dtype(dtype, [&](auto t) {
        return cooks<decltype(t)>(c.y, c.y_ld, (int)m, n_genes, n_groups, c.dd, dispersion, q, cutoff, min_replace, alpha_robust, max_cooks, arg_max,
                                  n_above, n_replace, trimmed_base, ResultMatrix{D, D_is_device, ld_D, (size_t)m, (size_t)n_genes}, bad_row, bad_col);
    });
}

// ---- K26: a general design (nb_design_kernels.hpp) ---------------------------------------------------------------------------------
namespace {

// every check of the design matrix; no HIP call
int check_design_matrix(const double *X, long long m, int p) {
    if (p < 2 || p > pilot::NB_DESIGN_MAX_COLS)
        return fail(PILOT_OT_EINVAL, "p=%d design columns must be in [2, %d]", p, pilot::NB_DESIGN_MAX_COLS);
    if (m - p < 1) return fail(PILOT_OT_EINVAL, "m=%lld samples and p=%d columns leave no residual degree of freedom", m, p);
    for (long long j = 0; j < m; ++j) {
        if (X[j * p] != 1.0) return fail(PILOT_OT_EINVAL, "X[%lld, 0]=%g: the first design column is ones", j, X[j * p]);
        for (int k = 1; k < p; ++k)
            if (!std::isfinite(X[j * p + k])) return fail(PILOT_OT_EINVAL, "X[%lld, %d]=%g must be finite", j, k, X[j * p + k]);
    }
    return PILOT_OT_OK;
}

// `staged`: what of a gene the call's kernel stages in LDS
int check_design_samples(long long m, int p, const char *staged = "counts, log size factors and design rows") {
    const int limit = pilot::nb_design_max_samples(p);
    return m > limit ? fail(PILOT_OT_ENOTSUP, "m=%lld samples: a gene's %s are staged in LDS, at most %d for p=%d", m, staged, limit, p) : PILOT_OT_OK;
}

// the size factors, their logarithms and X (m x p) behind each other in HBM: what both kernels read as `sf`
int upload_design_matrix(const double *sf, const double *X, size_t m, int p, double **dev) {
    std::vector<double> h((2 + (size_t)p) * m);
    for (size_t j = 0; j < m; ++j) { h[j] = sf[j]; h[m + j] = std::log(sf[j]); }
    for (size_t t = 0; t < m * (size_t)p; ++t) h[2 * m + t] = X[t];
    HIP_TRY(pilot::ws(pilot::WS_NB_SF, h.size(), dev));
    HIP_TRY(hipMemcpy(*dev, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
    return PILOT_OT_OK;
}

// body(std::integral_constant<int, P>()) for the P that is p (checked: 2 .. NB_DESIGN_MAX_COLS)
template <int P = 2, typename Body> int by_columns(int p, Body body) {
    if constexpr (P > pilot::NB_DESIGN_MAX_COLS) return fail(PILOT_OT_EINVAL, "p=%d", p);
    else return p == P ? body(std::integral_constant<int, P>()) : by_columns<P + 1>(p, body);
}

template <typename T, int P>
int design_dispersions(const void *y, long long ld, int m, int n_genes, const double *d_sf, const double *log_prior_mean, double prior_var,
                       double *log_disp, double *objective, double *beta, int *steps, int *flags, long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    const size_t G = (size_t)n_genes;
    double *d_out, *d_prior = nullptr;
    int *d_int;
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, (2 + (size_t)P) * G, &d_out));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, 2 * G, &d_int));
    if (log_prior_mean) {
        HIP_TRY(pilot::ws(pilot::WS_NB_PRIOR, G, &d_prior));
        HIP_TRY(hipMemcpy(d_prior, log_prior_mean, sizeof(double) * G, hipMemcpyHostToDevice));
    }
    if (int rc = launch_wave_per_gene(pilot::nb_design_dispersion_kernel<T, P>, n_genes, (2 + (size_t)P) * (size_t)m, static_cast<const T *>(y), ld,
                                      m, d_sf, d_prior, prior_var, d_out, d_out + G, d_out + 2 * G, d_int, d_int + G))
        return rc;
    HIP_TRY(fetch(log_disp, d_out, G));
    HIP_TRY(fetch(objective, d_out + G, G));
    if (beta) HIP_TRY(fetch(beta, d_out + 2 * G, G * P));
    HIP_TRY(fetch(steps, d_int, G));
    HIP_TRY(fetch(flags, d_int + G, G));
    return PILOT_OT_OK;
}

template <typename T, int P>
int design_fits(const void *y, long long ld, int m, int n_genes, const double *d_sf, const double *dispersion, double *beta, double *cov,
                double *loglik, int *steps, int *flags, long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    constexpr size_t TRI = pilot::NB_TRI<P>;
    const size_t G = (size_t)n_genes;
    double *d_disp, *d_out;                                  // d_out: beta | cov | loglik
    int *d_int;
    HIP_TRY(pilot::ws(pilot::WS_NB_PRIOR, G, &d_disp));
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, (P + TRI + 1) * G, &d_out));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, 2 * G, &d_int));
    HIP_TRY(hipMemcpy(d_disp, dispersion, sizeof(double) * G, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((pilot::nb_design_fit_kernel<T, P>), dim3((unsigned)((G + 255) / 256)), dim3(256), 0, nullptr, static_cast<const T *>(y), ld,
                       m, n_genes, d_sf, d_disp, d_out, d_out + P * G, d_out + (P + TRI) * G, d_int, d_int + G);
    HIP_TRY(hipGetLastError());
    HIP_TRY(fetch(beta, d_out, P * G));
    HIP_TRY(fetch(cov, d_out + P * G, TRI * G));
    HIP_TRY(fetch(loglik, d_out + (P + TRI) * G, G));
    HIP_TRY(fetch(steps, d_int, G));
    HIP_TRY(fetch(flags, d_int + G, G));
    return PILOT_OT_OK;
}

// K27.  d_sf and beta_mle have the shrunk column last; beta comes back in the caller's column order, info packed in the kernel's.
template <typename T, int P>
int design_shrink(const void *y, long long ld, int m, int n_genes, const double *d_sf, const double *dispersion, const double *beta_mle,
                  const double *far_end, double prior_scale, double other_scale, int coef, double *beta, double *objective, double *info,
                  int *flags, long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    constexpr size_t TRI = pilot::NB_TRI<P>;
    const size_t G = (size_t)n_genes;
    double *d_in, *d_out;                                    // d_in: dispersion | far_end | beta_mle;  d_out: beta | objective | info
    int *d_flags;
    HIP_TRY(pilot::ws(pilot::WS_NB_PRIOR, (2 + (size_t)P) * G, &d_in));
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, (P + 1 + TRI) * G, &d_out));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, G, &d_flags));
    HIP_TRY(hipMemcpy(d_in, dispersion, sizeof(double) * G, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_in + G, far_end, sizeof(double) * G, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_in + 2 * G, beta_mle, sizeof(double) * P * G, hipMemcpyHostToDevice));
    if (int rc = launch_wave_per_gene(pilot::nb_design_shrink_kernel<T, P>, n_genes, (2 + (size_t)P) * (size_t)m, static_cast<const T *>(y), ld, m,
                                      d_sf, d_in, d_in + 2 * G, d_in + G, prior_scale, 1.0 / (other_scale * other_scale), coef, d_out,
                                      d_out + P * G, d_out + (P + 1) * G, d_flags))
        return rc;
    HIP_TRY(fetch(beta, d_out, P * G));
    HIP_TRY(fetch(objective, d_out + P * G, G));
    HIP_TRY(fetch(info, d_out + (P + 1) * G, TRI * G));
    HIP_TRY(fetch(flags, d_flags, G));
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_nb_design_max_cols(void) { return pilot::NB_DESIGN_MAX_COLS; }

PILOT_API int pilot_ot_nb_design_max_samples(int p) {
    if (p < 2 || p > pilot::NB_DESIGN_MAX_COLS)
        return fail(PILOT_OT_EINVAL, "p=%d design columns must be in [2, %d]", p, pilot::NB_DESIGN_MAX_COLS);
    return pilot::nb_design_max_samples(p);
}

PILOT_API int pilot_ot_nb_design_dispersions(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *X,
                                             int p, const double *size_factors, const double *log_prior_mean, double prior_var,
                                             double *log_disp, double *objective, double *beta, int *steps, int *flags,
                                             int *n_not_converged, long long *bad_row, int *bad_col) {
    if (n_not_converged) *n_not_converged = 0;
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, false, nullptr, 1, nullptr, nullptr};
    if (int rc = prologue(
            c, !Y || !X || !size_factors || !log_disp || !objective || !steps || !flags, bad_row, bad_col,
            [&] { return log_prior_mean ? positive_finite("prior_var", prior_var, " when a prior is given") : PILOT_OT_OK; },
            [&] {
                if (int rc = check_design_matrix(X, m, p)) return rc;
                return check_design_samples(m, p);
            }))
        return rc;
    double *d_sf;
    if (int rc = upload_design_matrix(size_factors, X, (size_t)m, p, &d_sf)) return rc;
    if (int rc = by_dtype(dtype, [&](auto t) {
            return by_columns(p, [&](auto P) {
                return design_dispersions<decltype(t), decltype(P)::value>(c.y, c.y_ld, (int)m, n_genes, d_sf, log_prior_mean, prior_var, log_disp,
                                                                           objective, beta, steps, flags, bad_row, bad_col);
            });
        }))
        return rc;
    count_flag(flags, n_genes, pilot::NB_FLAG_NOT_CONVERGED, n_not_converged);
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_nb_design_fits(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *X, int p,
                                      const double *size_factors, const double *dispersion, double *beta, double *cov, double *loglik,
                                      int *steps, int *flags, int *n_not_converged, long long *bad_row, int *bad_col) {
    if (n_not_converged) *n_not_converged = 0;
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, false, nullptr, 1, nullptr, nullptr};
    if (int rc = prologue(c, !Y || !X || !size_factors || !dispersion || !beta || !cov || !loglik || !steps || !flags, bad_row, bad_col, no_check,
                          [&] {
                              if (int rc = check_dispersions(dispersion, n_genes, m)) return rc;
                              return check_design_matrix(X, m, p);
                          }))
        return rc;
    double *d_sf;
    if (int rc = upload_design_matrix(size_factors, X, (size_t)m, p, &d_sf)) return rc;
    if (int rc = by_dtype(dtype, [&](auto t) {
            return by_columns(p, [&](auto P) {
                return design_fits<decltype(t), decltype(P)::value>(c.y, c.y_ld, (int)m, n_genes, d_sf, dispersion, beta, cov, loglik, steps, flags,
                                                                    bad_row, bad_col);
            });
        }))
        return rc;
    count_flag(flags, n_genes, pilot::NB_FLAG_NOT_CONVERGED, n_not_converged);
    return PILOT_OT_OK;
}

// ---- K27: the shrunken coefficient under a general design (nb_design_shrink_kernel.hpp) ----------------------------------------------
PILOT_API int pilot_ot_nb_design_shrink(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *X, int p,
                                        int coef, const double *size_factors, const double *dispersion, const double *beta_mle,
                                        const double *far_end, double prior_scale, double other_scale, double *beta, double *objective,
                                        double *info, int *flags, int *n_at_bound, long long *bad_row, int *bad_col) {
    if (n_at_bound) *n_at_bound = 0;
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, false, nullptr, 1, dispersion, nullptr};
    if (int rc = prologue(
            c, !Y || !X || !size_factors || !dispersion || !beta_mle || !far_end || !beta || !objective || !info || !flags, bad_row, bad_col,
            [&] {
                if (int rc = positive_finite("prior_scale", prior_scale)) return rc;
                return positive_finite("other_scale", other_scale);
            },
            [&] {
                if (int rc = check_design_matrix(X, m, p)) return rc;
                if (coef < 1 || coef > p - 1)
                    return fail(PILOT_OT_EINVAL, "coef=%d must be in [1, p - 1 = %d] (the intercept is not shrunk)", coef, p - 1);
                for (int j = 0; j < n_genes; ++j)
                    if (!std::isfinite(far_end[j])) return fail(PILOT_OT_EINVAL, "far_end[%d]=%g must be finite", j, far_end[j]);
                return check_design_samples(m, p);
            }))
        return rc;
    // the shrunk column goes last: of X and of beta_mle (the kernel's column `at` is the caller's `from(at)`)
    const size_t M = (size_t)m, G = (size_t)n_genes, P = (size_t)p;
    const auto from = [&](size_t at) { return at == P - 1 ? (size_t)coef : at < (size_t)coef ? at : at + 1; };
    std::vector<double> Xk(M * P), mle(G * P);
    for (size_t j = 0; j < M; ++j)
        for (size_t k = 0; k < P; ++k) Xk[j * P + k] = X[j * P + from(k)];
    for (size_t g = 0; g < G; ++g)
        for (size_t k = 0; k < P; ++k) mle[g * P + k] = beta_mle[g * P + from(k)];
    double *d_sf;
    if (int rc = upload_design_matrix(size_factors, Xk.data(), M, p, &d_sf)) return rc;
    if (int rc = by_dtype(dtype, [&](auto t) {
            return by_columns(p, [&](auto Pc) {
                return design_shrink<decltype(t), decltype(Pc)::value>(c.y, c.y_ld, (int)m, n_genes, d_sf, dispersion, mle.data(), far_end,
                                                                       prior_scale, other_scale, coef, beta, objective, info, flags, bad_row,
                                                                       bad_col);
            });
        }))
        return rc;
    // the information back in the caller's column order (packed upper triangle, row by row)
    const size_t tri = P * (P + 1) / 2;
    const auto packed = [&](size_t i, size_t j) { return i * P - i * (i - 1) / 2 + (j - i); };
    std::vector<size_t> to(P);                               // the kernel's column of the caller's
    for (size_t k = 0; k < P; ++k) to[from(k)] = k;
    std::vector<double> row(tri);
    for (size_t g = 0; g < G; ++g) {
        double *mine = info + g * tri;
        for (size_t i = 0; i < P; ++i)
            for (size_t j = i; j < P; ++j) row[packed(i, j)] = mine[to[i] < to[j] ? packed(to[i], to[j]) : packed(to[j], to[i])];
        for (size_t t = 0; t < tri; ++t) mine[t] = row[t];
    }
    count_flag(flags, n_genes, pilot::NB_FLAG_AT_BOUND, n_at_bound);
    return PILOT_OT_OK;
}

// ---- K28: Cook's distances under a general design (nb_design_cooks_kernel.hpp) -------------------------------------------------------
namespace {

// cells are codes in [0, n_cells), and every row of a cell is bit-identical to the cell's first; no HIP call
int check_cells(const double *X, long long m, int p, const int *cells, int n_cells) {
    if (n_cells < 1 || n_cells > m) return fail(PILOT_OT_EINVAL, "n_cells=%d must be in [1, m = %lld]", n_cells, m);
    std::vector<long long> first((size_t)n_cells, -1);
    for (long long j = 0; j < m; ++j) {
        if (cells[j] < 0 || cells[j] >= n_cells) return fail(PILOT_OT_EINVAL, "cells[%lld]=%d outside [0, %d)", j, cells[j], n_cells);
        long long &f = first[(size_t)cells[j]];
        if (f < 0) f = j;
        else if (std::memcmp(X + j * p, X + f * p, sizeof(double) * (size_t)p) != 0)
            return fail(PILOT_OT_EINVAL, "cells[%lld]=%d: row %lld of X differs from row %lld, the first of that cell", j, cells[j], j, f);
    }
    return PILOT_OT_OK;
}

template <typename T, int P>
int design_cooks(const void *y, long long ld, int m, int n_genes, int n_cells, const DevDesign &dd, const double *d_sf, const double *dispersion,
                 const double *beta, double cutoff, int min_replace, double *alpha_robust, double *max_cooks, int *arg_max, int *n_above,
                 int *n_replace, double *trimmed_base, ResultMatrix D, ResultMatrix H, long long *bad_row, int *bad_col) {
    if (int rc = check_counts<T>(y, ld, m, n_genes, bad_row, bad_col)) return rc;
    const size_t G = (size_t)n_genes, M = (size_t)m;
    size_t Psort = 1;                                        // the sort buffer: the power of two >= m
    while (Psort < M) Psort <<= 1;
    double *d_in, *d_out;                                    // dispersion | beta;  the three double results | packed D | packed H (host ones)
    int *d_int;
    HIP_TRY(pilot::ws(pilot::WS_NB_PRIOR, (1 + (size_t)P) * G, &d_in));
    HIP_TRY(pilot::ws(pilot::WS_NB_OUT, 3 * G + D.tail() + H.tail(), &d_out));
    HIP_TRY(pilot::ws(pilot::WS_NB_FIT_INT, 3 * G, &d_int));
    HIP_TRY(hipMemcpy(d_in, dispersion, sizeof(double) * G, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_in + G, beta, sizeof(double) * P * G, hipMemcpyHostToDevice));
    D.place(d_out + 3 * G);
    H.place(d_out + 3 * G + D.tail());
    if (int rc = launch_wave_per_gene(pilot::nb_design_cooks_kernel<T, P>, n_genes, 2 * M + Psort, static_cast<const T *>(y), ld, m, n_cells,
                                      dd.order, dd.gof, dd.gstart, d_sf, d_in, d_in + G, cutoff, min_replace, n_genes, d_out, d_int, D.dev,
                                      D.ld(), H.dev, H.ld()))
        return rc;
    HIP_TRY(fetch(alpha_robust, d_out, G));
    HIP_TRY(fetch(max_cooks, d_out + G, G));
    HIP_TRY(fetch(trimmed_base, d_out + 2 * G, G));
    HIP_TRY(fetch(arg_max, d_int, G));
    HIP_TRY(fetch(n_above, d_int + G, G));
    HIP_TRY(fetch(n_replace, d_int + 2 * G, G));
    HIP_TRY(D.fetch());
    HIP_TRY(H.fetch());
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_nb_design_cooks(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *X, int p,
                                       const int *cells, int n_cells, const double *size_factors, const double *dispersion, const double *beta,
                                       double cutoff, int min_replace, double *alpha_robust, double *max_cooks, int *arg_max, int *n_above,
                                       int *n_replace, double *trimmed_base, void *D, int D_is_device, long long ld_D, void *H, int H_is_device,
                                       long long ld_H, long long *bad_row, int *bad_col) {
    Call c{Y, Y_is_device, dtype, m, n_genes, ld, size_factors, false, nullptr, 1, dispersion, nullptr};
    if (int rc = prologue(
            c, !Y || !X || !cells || !size_factors || !dispersion || !beta || !alpha_robust || !max_cooks || !arg_max || !n_above || !n_replace ||
                   !trimmed_base,
            bad_row, bad_col,
            [&] {
                if (int rc = positive_finite("cutoff", cutoff)) return rc;
                if (min_replace < pilot::NB_COOKS_MIN_GROUP)
                    return fail(PILOT_OT_EINVAL, "min_replace=%d: at least %d (smaller cells have no Cook's distance to compare)", min_replace,
                                pilot::NB_COOKS_MIN_GROUP);
                if (D && ld_D < n_genes) return fail(PILOT_OT_EINVAL, "ld_D=%lld is smaller than n_genes=%d", ld_D, n_genes);
                return H && ld_H < n_genes ? fail(PILOT_OT_EINVAL, "ld_H=%lld is smaller than n_genes=%d", ld_H, n_genes) : PILOT_OT_OK;
            },
            [&] {
                if (int rc = check_design_matrix(X, m, p)) return rc;
                if (int rc = check_cells(X, m, p, cells, n_cells)) return rc;
                if (int rc = sort_samples(m, cells, n_cells, size_factors, "cell", c.d)) return rc;
                for (int j = 0; j < n_genes; ++j) {
                    if (std::isnan(dispersion[j])) continue;
                    for (int t = 0; t < p; ++t) {
                        const double v = beta[(long long)j * p + t];
                        if (!std::isfinite(v)) return fail(PILOT_OT_EINVAL, "beta[%d, %d]=%g must be finite where the gene has a dispersion", j, t, v);
                    }
                }
                return check_design_samples(m, p, "counts, normalised counts and sort buffer");
            }))
        return rc;
    if (int rc = upload_order(c.d, c.dd)) return rc;
    double *d_sf;
    if (int rc = upload_design_matrix(size_factors, X, (size_t)m, p, &d_sf)) return rc;
    return by_dtype(dtype, [&](auto t) {
        return by_columns(p, [&](auto P) {
            return design_cooks<decltype(t), decltype(P)::value>(
                c.y, c.y_ld, (int)m, n_genes, n_cells, c.dd, d_sf, dispersion, beta, cutoff, min_replace, alpha_robust, max_cooks, arg_max, n_above,
                n_replace, trimmed_base, ResultMatrix{D, D_is_device, ld_D, (size_t)m, (size_t)n_genes},
                ResultMatrix{H, H_is_device, ld_H, (size_t)m, (size_t)n_genes}, bad_row, bad_col);
        });
    });
}
