// K24: the regularised log transform of pseudobulk counts (DESeq2's rlog, Love, Huber, Anders 2014; include/pilot_ot.h,
// "negative-binomial GLM", pilot_ot_nb_rlog).  Per gene a negative-binomial GLM with one coefficient a sample and an
// intercept, eta_j = b0 + b_j + log s_j, at the gene's dispersion a, with a ridge on the sample coefficients:
//   P(b0, b) = sum_j [c_j eta_j - (c_j + 1/a) log1p(a e^{eta_j})] - lambda/2 sum_j b_j^2 - lambda0/2 b0^2
// P is strictly concave: the estimate is its one maximiser, whatever the path.  K22 and K23 decouple by group; this does not, but the
// Hessian is an arrowhead (a diagonal h_j = w_j + lambda bordered by w), so a Newton step costs four sums:
//   mu = e^eta,  r = (c - mu) / (1 + a mu),  w = mu (1 + a c) / (1 + a mu)^2,  g = r - lambda b,  h = w + lambda
//   d0  = (sum r - lambda0 b0 - sum w g / h) / (sum w + lambda0 - sum w^2 / h),     d_j = (g_j - w_j d0) / h_j
//
// nb_rlog_kernel   one wave per gene, THE SAMPLES ALONG THE LANES: lane l owns samples l, l + 64, ...  The gene's c_j, log s_j and
//                  b_j are staged in LDS and a lane reads and writes its own samples only, so the kernel has no barrier.  Every
//                  sum is a per-lane partial in sample order, then lanes_sum (reduce.hpp); no floating-point atomic.  An
//                  iteration is three passes: the four sums; the line search (t halved from 1, at most NB_RLOG_MAX_HALVINGS
//                  times, until P does not fall); the step.  The d_j are recomputed in the last two instead of kept (a fourth
//                  array would put the 4096-sample limit past 96 KiB).  Whether P falls is read from the CHANGE of P,
//                    sum_j [c D_j - (c + 1/a) log1p(rho_j expm1(D_j)) - lambda/2 t d_j (2 b_j + t d_j)] - lambda0/2 t d0 (2 b0 + t d0),
//                    D_j = t (d0 + d_j),  rho_j = a mu_j / (1 + a mu_j),
//                  which is P(trial) - P(current) term by term without the cancellation of two sums of size |P|: near the optimum
//                  the gain of a step is far below an ulp of P, and a comparison of two rounded P would halve good steps at
//                  random and could stop short.  A non-finite change (exp overflows on a long first step) counts as a fall; a step
//                  that is within the tolerance at t = 1 is taken whole, unsearched (its change of P is below its own rounding).
//                  Stops when max(|t d0|, max_j |t d_j|) <= NB_RLOG_TOL after the step; NB_RLOG_MAX_ITERS iterations set
//                  NB_FLAG_NOT_CONVERGED.  LDS: 24 m bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "nb_glm_kernels.hpp"

namespace pilot {

constexpr int NB_RLOG_MAX_ITERS = 100;
constexpr int NB_RLOG_MAX_HALVINGS = 20;
constexpr double NB_RLOG_TOL = 1e-10;
constexpr double NB_RLOG_LN2 = 0.69314718055994530942;
constexpr double NB_RLOG_INTERCEPT_RIDGE = 1e-6;    // lambda0 = 1e-6 ln2^2: the intercept is all but free

// what the passes share of a gene
struct NbRlogGene {
    int m;
    double alpha, inv_alpha, lambda, lambda0;
};

// the terms of sample j at (b0, b): w, g, h and rho = alpha mu / (1 + alpha mu); returns r
__device__ inline double nb_rlog_terms(const NbRlogGene &G, double c, double eta, double b, double &w, double &g, double &h, double &rho) {
    const double mu = exp(eta), inv = 1.0 / (1.0 + G.alpha * mu), r = (c - mu) * inv;
    rho = G.alpha * mu * inv;
    w = (mu * inv) * ((1.0 + G.alpha * c) * inv);            // (in two factors: mu / (1 + a mu) <= 1 / a where (1 + a mu)^2 would overflow)
    g = r - G.lambda * b;
    h = w + G.lambda;
    return r;
}

// the Newton step's intercept part d0 at (b0, sb)
__device__ inline double nb_rlog_d0(const NbRlogGene &G, const double *sc, const double *sl, const double *sb, double b0, int lane) {
    double s_r = 0.0, s_w = 0.0, s_wg = 0.0, s_ww = 0.0;
    for (int p = lane; p < G.m; p += 64) {
        double w, g, h, rho;
        const double b = sb[p], r = nb_rlog_terms(G, sc[p], b0 + b + sl[p], b, w, g, h, rho);
        s_r += r;
        s_w += w;
        s_wg += w * g / h;
        s_ww += w * w / h;
    }
    s_r = lanes_sum(s_r);
    s_w = lanes_sum(s_w);
    s_wg = lanes_sum(s_wg);
    s_ww = lanes_sum(s_ww);
    return (s_r - G.lambda0 * b0 - s_wg) / (s_w + G.lambda0 - s_ww);
}

// P(b0 + t d0, b + t d) - P(b0, b), and dmax = max_j |d_j|
__device__ inline double nb_rlog_change(const NbRlogGene &G, const double *sc, const double *sl, const double *sb, double b0, double d0,
                                        double t, int lane, double &dmax) {
    double part = 0.0, big = 0.0;
    for (int p = lane; p < G.m; p += 64) {
        double w, g, h, rho;
        const double c = sc[p], b = sb[p];
        nb_rlog_terms(G, c, b0 + b + sl[p], b, w, g, h, rho);
        const double d = (g - w * d0) / h, D = t * (d0 + d), td = t * d;
        part += c * D - (c + G.inv_alpha) * log1p(rho * expm1(D)) - 0.5 * G.lambda * td * (2.0 * b + td);
        big = fabs(d) > big ? fabs(d) : big;
    }
    dmax = lanes_reduce(big, Max{});
    const double t0 = t * d0;
    return lanes_sum(part) - 0.5 * G.lambda0 * t0 * (2.0 * b0 + t0);
}

// b += t d
__device__ inline void nb_rlog_step(const NbRlogGene &G, const double *sc, const double *sl, double *sb, double b0, double d0, double t, int lane) {
    for (int p = lane; p < G.m; p += 64) {
        double w, g, h, rho;
        const double b = sb[p];
        nb_rlog_terms(G, sc[p], b0 + b + sl[p], b, w, g, h, rho);
        sb[p] = fma(t, (g - w * d0) / h, b);
    }
}

// Grid: n_genes workgroups of one wave.  Dynamic LDS: 3 m doubles.  sf: the m size factors, then their m logarithms.  out: m x n_genes
// with leading dimension ld_out, (b0 + b_j) / ln 2; intercept: b0 / ln 2.  A NaN dispersion leaves its gene out (NaN everywhere,
// steps = flags = 0); a gene of zeros gives 0 in every sample and a NaN intercept (steps = flags = 0).
template <typename T>
__global__ void __launch_bounds__(64) nb_rlog_kernel(const T *__restrict__ Y, long long ld, int m, const double *__restrict__ sf,
                                                      const double *__restrict__ dispersion, double lambda, double lambda0,
                                                      double *__restrict__ out, long long ld_out, double *__restrict__ intercept,
                                                      int *__restrict__ steps_out, int *__restrict__ flags_out) {
    extern __shared__ double nb_rlog_lds[];
    double *sc = nb_rlog_lds, *sl = sc + m, *sb = sl + m;
    const int gene = blockIdx.x, lane = threadIdx.x;
    const double alpha = dispersion[gene];
    double qsum = 0.0;
    if (alpha == alpha)
        for (int p = lane; p < m; p += 64) {
            const double c = rint((double)Y[(long long)p * ld + gene]);
            sc[p] = c;
            sl[p] = sf[m + p];
            sb[p] = 0.0;
            qsum += c / sf[p];
        }
    qsum = lanes_sum(qsum);
    if (!(qsum > 0.0)) {                                     // (uniform) a NaN dispersion, or counts that are all zero
        const double fill = alpha == alpha ? 0.0 : __builtin_nan("");
        for (int p = lane; p < m; p += 64) out[(long long)p * ld_out + gene] = fill;
        if (lane == 0) {
            intercept[gene] = __builtin_nan("");
            steps_out[gene] = flags_out[gene] = 0;
        }
        return;
    }

    const NbRlogGene G = {m, alpha, 1.0 / alpha, lambda, lambda0};
    double b0 = log(qsum / (double)m);
    int it = 0, flags = NB_FLAG_NOT_CONVERGED;
    while (it < NB_RLOG_MAX_ITERS) {
        ++it;
        const double d0 = nb_rlog_d0(G, sc, sl, sb, b0, lane);
        double t = 1.0, moved;
        for (int halvings = 0;; ++halvings) {
            double dmax;
            const double change = nb_rlog_change(G, sc, sl, sb, b0, d0, t, lane, dmax);
            moved = fabs(d0) > dmax ? fabs(d0) : dmax;
            // (a whole step within the tolerance is taken whole: the change of P is below its own rounding there)
            if ((__builtin_isfinite(change) && change >= 0.0) || moved <= NB_RLOG_TOL || halvings == NB_RLOG_MAX_HALVINGS) break;
            t *= 0.5;
        }
        nb_rlog_step(G, sc, sl, sb, b0, d0, t, lane);
        b0 = fma(t, d0, b0);
        if (t * moved <= NB_RLOG_TOL) { flags = 0; break; }  // (t is a power of two: t |d| is |t d|; a NaN never stops)
    }
    for (int p = lane; p < m; p += 64) out[(long long)p * ld_out + gene] = (b0 + sb[p]) / NB_RLOG_LN2;
    if (lane == 0) {
        intercept[gene] = b0 / NB_RLOG_LN2;
        steps_out[gene] = it;
        flags_out[gene] = flags;
    }
}

}  // namespace pilot
