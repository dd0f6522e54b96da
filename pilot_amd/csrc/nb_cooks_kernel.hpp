// K25: the Cook's distances of DESeq2's outlier handling for the one-factor design of K22 (the rule is this
// library's statement, unpinned).  Y, order / gof / ss / gstart as in nb_glm_kernels.hpp; c = rint(Y), q_p = c_p / s_p, k groups.
//
// nb_cooks_kernel  one wave per gene.  The gene's c_p and q_p are staged once in LDS in sorted (group, sample) order; a third buffer
//                  of P = the power of two >= m doubles holds whatever is being sorted, padded with +inf, by K21's bitonic network
//                  (rs_bitonic_lds with a plain double as the record).  With tm(x, d) the mean of the sorted x without its d lowest
//                  and d highest values:
//                    trimmed_base = tm(q of all samples, m / 5)
//                    per group of n >= 3 samples, (d, scale) = nb_cooks_trim(n):  t = tm(q_g, d),  v_g = scale tm((q_g - t)^2, d)
//                    alpha_R = max((max_g v_g - mean q) / (mean q)^2, 0.04)
//                    mu_p = max(s_p qfit[g(p)], minmu),  w_p = mu_p / (1 + alpha mu_p),  h_p = w_p / sum_{i in g(p)} w_i
//                    D_p = (c_p - mu_p)^2 / (mu_p + alpha_R mu_p^2)  h_p / (k (1 - h_p)^2),   NaN in a group of one sample
//                  The squared deviations are formed in place on the sorted group and sorted again; once a group's order statistics
//                  are taken its q_p are dead and the slots keep h_p, so nothing per group is stored.  LDS: 8 (2 m + P) bytes,
//                  96 KiB at m = 4096.
//                  Every sum is a per-lane partial over p = first + lane, + 64, ... closed by lanes_sum; the maximum and its lowest
//                  sample index by lanes_best(LowestMax).  Nothing depends on the other genes of the launch, on the storage type or on
//                  where Y lives: a gene gives the same bits alone and in any batch.
#pragma once
#include <hip/hip_runtime.h>

#include "nb_glm_kernels.hpp"
#include "rank_sums_kernels.hpp"

namespace pilot {

constexpr double NB_COOKS_MIN_ROBUST_DISP = 0.04;
constexpr int NB_COOKS_MIN_GROUP = 3;        // a group takes part in the robust variance and in max_cooks from this size
constexpr int NB_COOKS_BASE_TRIM_DIV = 5;    // trimmed_base drops floor(m / 5) = floor(0.2 m) values from each end

// how many values a group of n samples drops from each end (floor(n r), r = 1/3, 1/4, 1/8) and the scale of its trimmed variance
__host__ __device__ inline void nb_cooks_trim(int n, int &drop, double &scale) {
    if (n <= 3) { drop = n / 3; scale = 2.04; }
    else if (n <= 23) { drop = n / 4; scale = 1.86; }
    else { drop = n / 8; scale = 1.51; }
}

struct NbSortKey {
    typedef double Rec;
    __device__ static double value(double x) { return x; }
};

// ascending sort of s[0 .. n), written by the wave (no barrier since needed); s holds the power of two >= n.  Ends on a barrier.
__device__ inline void nb_sort(double *s, int n, int lane) {
    int P = 1;
    while (P < n) P <<= 1;
    for (int p = n + lane; p < P; p += 64) s[p] = __builtin_inf();
    __syncthreads();
    rs_bitonic_lds<NbSortKey, 64>(s, P, 0, 2, P);
}

// mean of s[d .. n - d) of the sorted s
__device__ inline double nb_trimmed_mean(const double *s, int n, int d, int lane) {
    double part = 0.0;
    for (int p = d + lane; p < n - d; p += 64) part += s[p];
    return lanes_sum(part) / (double)(n - 2 * d);
}

// Grid: n_genes workgroups of one wave.  Dynamic LDS: 2 m + P doubles.  qfit: n_genes x k (pilot_ot_nb_group_fits' q).
// out_d: alpha_robust | max_cooks | trimmed_base, out_i: arg_max | n_above | n_replace, each n_genes.  D: nullable, m x n_genes with
// leading dimension ldD, sample-major in the samples' own order.
template <typename T>
__global__ void __launch_bounds__(64) nb_cooks_kernel(const T *__restrict__ Y, long long ld, int m, int k, const int *__restrict__ order,
                                                       const int *__restrict__ gof, const double *__restrict__ ss,
                                                       const int *__restrict__ gstart, const double *__restrict__ dispersion,
                                                       const double *__restrict__ qfit, double cutoff, int min_replace, int n_genes,
                                                       double *__restrict__ out_d, int *__restrict__ out_i, double *__restrict__ D,
                                                       long long ldD) {
    extern __shared__ double nb_lds[];
    double *sc = nb_lds, *sq = sc + m, *srt = sq + m;
    const int gene = blockIdx.x, lane = threadIdx.x;
    const double nan = __builtin_nan("");

    int any = 0;
    double part = 0.0;
    for (int p = lane; p < m; p += 64) {
        const double c = rint((double)Y[(long long)order[p] * ld + gene]), q = c / ss[p];
        sc[p] = c;
        sq[p] = q;
        srt[p] = q;
        part += q;
        any |= c > 0.0;
    }
    any = lanes_reduce(any, Max{});
    const double alpha = dispersion[gene];
    if (!any || alpha != alpha) {
        if (lane == 0) {
            out_d[gene] = out_d[n_genes + gene] = out_d[2 * (long long)n_genes + gene] = nan;
            out_i[gene] = -1;
            out_i[n_genes + gene] = out_i[2 * (long long)n_genes + gene] = 0;
        }
        if (D)
            for (int p = lane; p < m; p += 64) D[(long long)order[p] * ldD + gene] = nan;
        return;
    }
    const double mean_q = lanes_sum(part) / (double)m;
    nb_sort(srt, m, lane);
    const double trimmed_base = nb_trimmed_mean(srt, m, m / NB_COOKS_BASE_TRIM_DIV, lane);
    __syncthreads();                                             // srt is read; the groups write it next

    const double *qg = qfit + (long long)gene * k;
    double v_robust = 0.0;
    int have = 0;
    for (int g = 0; g < k; ++g) {
        const int a = gstart[g], n = gstart[g + 1] - a;
        if (n >= NB_COOKS_MIN_GROUP) {
            int drop;
            double scale;
            nb_cooks_trim(n, drop, scale);
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
            __syncthreads();
            v_robust = have && v_robust > v ? v_robust : v;
            have = 1;
        }
        // the group's q_p are dead now: the slots take h_p
        const double q = qg[g];
        double sw = 0.0;
        for (int i = lane; i < n; i += 64) {
            double mu = ss[a + i] * q;
            mu = mu > NB_MIN_MU ? mu : NB_MIN_MU;
            const double w = mu / (1.0 + alpha * mu);
            sq[a + i] = w;
            sw += w;
        }
        sw = lanes_sum(sw);
        for (int i = lane; i < n; i += 64) sq[a + i] = sq[a + i] / sw;   // (a lane reads what it wrote)
    }
    __syncthreads();                                             // the pass below walks p by lane, not a + i
    double alpha_robust = nan;
    if (have) {
        alpha_robust = (v_robust - mean_q) / (mean_q * mean_q);
        alpha_robust = alpha_robust > NB_COOKS_MIN_ROBUST_DISP ? alpha_robust : NB_COOKS_MIN_ROBUST_DISP;
    }

    double best = -__builtin_inf(), best_c = -1.0;
    int best_at = 0x7fffffff, n_replace = 0;
    for (int p = lane; p < m; p += 64) {
        const int g = gof[p], n = gstart[g + 1] - gstart[g], sample = order[p];
        const double c = sc[p], h = sq[p];
        double mu = ss[p] * qg[g];
        mu = mu > NB_MIN_MU ? mu : NB_MIN_MU;
        const double r = c - mu, one_h = 1.0 - h;
        const double d = n == 1 ? nan : r * r / (mu + alpha_robust * mu * mu) * h / ((double)k * one_h * one_h);
        if (D) D[(long long)sample * ldD + gene] = d;
        if (have && n >= NB_COOKS_MIN_GROUP && (d > best || (d == best && sample < best_at))) { best = d; best_at = sample; best_c = c; }
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
