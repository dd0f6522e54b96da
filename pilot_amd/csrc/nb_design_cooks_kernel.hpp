// K28: K25's Cook's distances for the GENERAL design of K26 (the rule is this library's statement, unpinned).  Y as in
// nb_glm_kernels.hpp; c = rint(Y), q_j = c_j / s_j.  X is m x P with P a template parameter (nb_design_kernels.hpp).  The "groups" of
// K25 are CELLS: maximal sets of samples with bit-identical rows of X, numbered by first appearance (the host finds and checks them);
// order / gof / gstart are K25's, with the cells as the groups.
//
// nb_design_cooks_kernel<T, P>  one wave per gene.  c_j and q_j are staged once in LDS in sorted (cell, sample) order beside the sort
//                  buffer of P' = the power of two >= m doubles, as K25: 8 (2 m + P') bytes.  X and log s are NOT staged (beside the
//                  sort buffer they do not fit at P = 8, m = 1228): a lane reads the rows of its own samples from global memory, 8 P
//                  bytes contiguous each and at most 78 KB a launch, which every gene of the launch reads again.
//                    trimmed_base = tm(q of all samples, m / 5)
//                    v = max over the cells of n >= 3 samples of K25's scale tm((q_cell - tm(q_cell, d))^2, d), (d, scale) =
//                        nb_cooks_trim(n);  without such a cell v = 1.51 tm((q - tm(q, m / 8))^2, m / 8) over all samples
//                    alpha_R = max((v - mean q) / (mean q)^2, 0.04)
//                    mu_j = max(exp(x_j^T beta + log s_j), minmu),  w_j = mu_j / (1 + alpha mu_j),  M = X^T W X + lambda I
//                    h_j = w_j x_j^T M^-1 x_j,   D_j = (c_j - mu_j)^2 / (mu_j + alpha_R mu_j^2)  h_j / (P (1 - h_j)^2)
//                  M is formed as per-lane partials of the packed upper triangle over p = lane, lane + 64, ..., every entry closed by
//                  lanes_sum, then factored and inverted by every lane alike in registers (nb_cholesky, nb_cholesky_inverse); a lane
//                  forms the h_j of its own samples.  Once the order statistics are taken the q_j are dead and their slots keep mu_j.
//                  max_cooks, arg_max, n_above and n_replace as K25, over the samples of cells with n >= 3 (none: NaN, -1, 0; the
//                  distances are still computed, and with the ridge h_j < 1: no NaN rule for a cell of one).
//                  Nothing depends on the other genes of the launch, on the storage type or on where Y lives.
#pragma once
#include <hip/hip_runtime.h>

#include "nb_cooks_kernel.hpp"
#include "nb_design_kernels.hpp"

namespace pilot {

constexpr int NB_DESIGN_COOKS_FALLBACK_TRIM_DIV = 8;      // without a cell of 3: trimmedVariance over all samples, trim 1/8
constexpr double NB_DESIGN_COOKS_FALLBACK_SCALE = 1.51;

// x^T S x for the packed upper triangle S of a symmetric matrix
template <int P> __device__ inline double nb_design_quad(const double (&S)[NB_TRI<P>], const double (&x)[P]) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double row = S[nb_tri<P>(i, i)] * x[i];
#pragma unroll
        for (int j = 0; j < P; ++j)
            if (j > i) row = fma(2.0 * S[nb_tri<P>(i, j > i ? j : i)], x[j], row);
        v = fma(x[i], row, v);
    }
    return v;
}

// Grid: n_genes workgroups of one wave.  Dynamic LDS: 2 m + P' doubles.  sf: the m size factors, then their m logarithms, then X
// (m x P, row-major), all in the samples' own order.  k cells.  beta: n_genes x P (pilot_ot_nb_design_fits' at `dispersion`).
// out_d: alpha_robust | max_cooks | trimmed_base, out_i: arg_max | n_above | n_replace, each n_genes.  D, H: nullable, m x n_genes with
// leading dimensions ldD, ldH, sample-major in the samples' own order.
template <typename T, int P>
__global__ void __launch_bounds__(64) nb_design_cooks_kernel(const T *__restrict__ Y, long long ld, int m, int k, const int *__restrict__ order,
                                                              const int *__restrict__ gof, const int *__restrict__ gstart,
                                                              const double *__restrict__ sf, const double *__restrict__ dispersion,
                                                              const double *__restrict__ beta_in, double cutoff, int min_replace, int n_genes,
                                                              double *__restrict__ out_d, int *__restrict__ out_i, double *__restrict__ D,
                                                              long long ldD, double *__restrict__ H, long long ldH) {
    extern __shared__ double nb_lds[];
    double *sc = nb_lds, *sq = sc + m, *srt = sq + m;
    const int gene = blockIdx.x, lane = threadIdx.x;
    const double nan = __builtin_nan("");
    const double *sl = sf + m, *X = sf + 2 * m;

    int any = 0;
    double part = 0.0;
    for (int p = lane; p < m; p += 64) {
        const int sample = order[p];
        const double c = rint((double)Y[(long long)sample * ld + gene]), q = c / sf[sample];
        sc[p] = c;
        sq[p] = q;
        srt[p] = q;
        part += q;
        any |= c > 0.0;
    }
    any = lanes_reduce(any, Max{});
    const double alpha = dispersion[gene];
    double beta[P];
    int fitted = 1;
#pragma unroll
    for (int t = 0; t < P; ++t) {
        beta[t] = beta_in[(long long)gene * P + t];
        fitted &= __builtin_isfinite(beta[t]);
    }
    if (!any || alpha != alpha || !fitted) {
        if (lane == 0) {
            out_d[gene] = out_d[n_genes + gene] = out_d[2 * (long long)n_genes + gene] = nan;
            out_i[gene] = -1;
            out_i[n_genes + gene] = out_i[2 * (long long)n_genes + gene] = 0;
        }
        for (int p = lane; p < m; p += 64) {
            if (D) D[(long long)order[p] * ldD + gene] = nan;
            if (H) H[(long long)order[p] * ldH + gene] = nan;
        }
        return;
    }
    const double mean_q = lanes_sum(part) / (double)m;
    nb_sort(srt, m, lane);
    const double trimmed_base = nb_trimmed_mean(srt, m, m / NB_COOKS_BASE_TRIM_DIV, lane);

    // the robust variance: K25's expression per cell of 3 or more; srt keeps the sorted q of all samples until a cell writes it
    double v_robust = 0.0;
    int have = 0;
    for (int g = 0; g < k; ++g) {
        const int a = gstart[g], n = gstart[g + 1] - a;
        if (n < NB_COOKS_MIN_GROUP) continue;
        int drop;
        double scale;
        nb_cooks_trim(n, drop, scale);
        __syncthreads();                                         // srt is read; the cell writes it next
        for (int i = lane; i < n; i += 64) srt[i] = sq[a + i];
        nb_sort(srt, n, lane);
        const double t = nb_trimmed_mean(srt, n, drop, lane);
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            const double dev = srt[i] - t;
            srt[i] = dev * dev;
        }
        nb_sort(srt, n, lane);
        const double v = scale * nb_trimmed_mean(srt, n, drop, lane);
        v_robust = have && v_robust > v ? v_robust : v;
        have = 1;
    }
    if (!have) {                                                 // no cell of 3: the trimmed variance over all samples
        const int drop = m / NB_DESIGN_COOKS_FALLBACK_TRIM_DIV;
        const double t = nb_trimmed_mean(srt, m, drop, lane);
        __syncthreads();
        for (int i = lane; i < m; i += 64) {
            const double dev = srt[i] - t;
            srt[i] = dev * dev;
        }
        nb_sort(srt, m, lane);
        v_robust = NB_DESIGN_COOKS_FALLBACK_SCALE * nb_trimmed_mean(srt, m, drop, lane);
    }
    double alpha_robust = (v_robust - mean_q) / (mean_q * mean_q);
    alpha_robust = alpha_robust > NB_COOKS_MIN_ROBUST_DISP ? alpha_robust : NB_COOKS_MIN_ROBUST_DISP;

    // M = X^T W X + lambda I: a lane's partial over its own samples, every entry closed across the lanes.  The q_p are dead: the slots
    // take mu_p (a lane reads below what it wrote itself)
    double M[NB_TRI<P>], S[NB_TRI<P>];
#pragma unroll
    for (int t = 0; t < NB_TRI<P>; ++t) M[t] = 0.0;
    for (int p = lane; p < m; p += 64) {
        const int sample = order[p];
        double x[P];
#pragma unroll
        for (int t = 0; t < P; ++t) x[t] = X[(long long)sample * P + t];
        double mu = exp(nb_design_eta<P>(x, beta, sl[sample]));
        mu = mu > NB_MIN_MU ? mu : NB_MIN_MU;
        sq[p] = mu;
        nb_design_rank1<P>(M, x, mu / (1.0 + alpha * mu));
    }
#pragma unroll
    for (int t = 0; t < NB_TRI<P>; ++t) M[t] = lanes_sum(M[t]);
#pragma unroll
    for (int t = 0; t < P; ++t) M[nb_tri<P>(t, t)] += NB_DESIGN_RIDGE;
    nb_cholesky<P>(M);
    nb_cholesky_inverse<P>(M, S);

    double best = -__builtin_inf(), best_c = -1.0;
    int best_at = 0x7fffffff, n_replace = 0;
    for (int p = lane; p < m; p += 64) {
        const int g = gof[p], n = gstart[g + 1] - gstart[g], sample = order[p];
        double x[P];
#pragma unroll
        for (int t = 0; t < P; ++t) x[t] = X[(long long)sample * P + t];
        const double c = sc[p], mu = sq[p];
        const double h = mu / (1.0 + alpha * mu) * nb_design_quad<P>(S, x);
        const double r = c - mu, one_h = 1.0 - h;
        const double d = r * r / (mu + alpha_robust * mu * mu) * h / ((double)P * one_h * one_h);
        if (D) D[(long long)sample * ldD + gene] = d;
        if (H) H[(long long)sample * ldH + gene] = h;
        if (n >= NB_COOKS_MIN_GROUP && (d > best || (d == best && sample < best_at))) { best = d; best_at = sample; best_c = c; }
        n_replace += d > cutoff && n >= min_replace;
    }
    double top = best;
    int top_at = best_at;
    lanes_best(top, top_at, LowestMax{});
    const double top_c = lanes_reduce(have && best_at == top_at ? best_c : -1.0, Max{});
    int n_above = 0;
    for (int p = lane; p < m; p += 64) n_above += have && sc[p] > top_c;
    n_above = lanes_sum(n_above);
    n_replace = lanes_sum(n_replace);
    if (lane == 0) {
        out_d[gene] = alpha_robust;
        out_d[n_genes + gene] = have ? top : nan;
        out_d[2 * (long long)n_genes + gene] = trimmed_base;
        out_i[gene] = have ? top_at : -1;
        out_i[n_genes + gene] = n_above;
        out_i[2 * (long long)n_genes + gene] = n_replace;
    }
}

}  // namespace pilot
