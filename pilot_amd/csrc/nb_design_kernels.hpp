// K26: the negative-binomial GLM of DESeq2 for a GENERAL design (an m x p matrix X whose first column is ones: covariates beside the
// group indicator; include/pilot_ot.h, "negative-binomial GLM for a general design").  With a covariate nothing
// decouples by group as in K22: the mean of a sample is mu_j = s_j exp(x_j^T beta) with one p-vector beta per gene, X^T W X is a full
// p x p matrix and the Cox-Reid term is log det X^T W X.  Y is samples x genes, row-major; c = rint(Y).  All arithmetic is f64.
//
// P IS A TEMPLATE PARAMETER: beta, the gradient and the packed upper triangle (P (P + 1) / 2 words) of the p x p matrices live in
// registers.  Every loop over them has the constant bound P and is fully unrolled, with the triangular conditions (k < j, ...) as
// `if`s that fold away once the indices are constants; an index that stayed a variable would send the array to scratch.
//
// nb_design_solve      the inner fit, by one thread: the maximiser of
//                        l(beta) = sum_j [c_j eta_j - (c_j + 1/a) log1p(a e^{eta_j})] - lambda/2 |beta|^2,   eta_j = x_j^T beta + log s_j
//                      (the penalised log likelihood up to terms without beta; strictly concave).  Newton steps with the observed
//                      information H = sum_j w_j x_j x_j^T + lambda I, w = mu (1 + a c) / (1 + a mu)^2, and the score
//                      g = sum_j x_j (c_j - mu_j) / (1 + a mu_j) - lambda beta, solved by a Cholesky factorisation; the step is halved
//                      from 1, at most NB_DESIGN_MAX_HALVINGS times, while l would fall.  As in K24 that is read from the CHANGE of l,
//                        sum_j [c D_j - (c + 1/a) log1p(rho_j expm1(D_j))] - lambda/2 sum_k t d_k (2 beta_k + t d_k),
//                        D_j = t x_j^T d,  rho_j = a mu_j / (1 + a mu_j),
//                      term by term (a non-finite change counts as a fall; a step within the tolerance at t = 1 is taken whole).
//                      Stops once max_k |t d_k| <= NB_DESIGN_TOL; NB_DESIGN_MAX_ITERS steps set NB_FLAG_NOT_CONVERGED.  The samples
//                      come through a functor, so that both kernels walk them in sample order with the same arithmetic.
// nb_design_dispersion_kernel<P>   one wave per gene, A LANE IS A GRID POINT (K22's shape).  c, log s and X are staged once in LDS and
//                      read as broadcasts.  Every lane runs the inner fit at its own x = log(alpha), then
//                        L(x) = sum_j [lgamma(c + r) - lgamma(r) - (c + r) log1p(a mu~) + c log(a mu~)] - 1/2 log det(X^T W X)
//                               [- (x - prior_mean)^2 / (2 prior_var)],   mu~ = max(mu, minmu), W = diag(mu~ / (1 + a mu~)),
//                      the determinant from the Cholesky factor.  Round 0 starts every lane from (log max(mean c / s, minmu), 0, ...);
//                      a later round from the coefficients of the previous round's winner, which are wave-uniform.  No floating-point
//                      sum crosses lanes: the argmax of nb_grid_rounds is the only cross-lane step of the search (the step count
//                      is an integer sum), so a gene gives the same bits alone and in any batch.  LDS: 8 m (2 + P) bytes.
// nb_design_fit_kernel<P>   the final fit, one lane per gene, genes along the lanes so that a sample's row is read coalesced; log s and
//                      X are read wave-uniformly.  beta, Sigma = (X^T W X + lambda I)^-1 with W at mu~ (packed upper triangle, by
//                      inverting the Cholesky factor) and the unpenalised, unfloored log likelihood.
#pragma once
#include <hip/hip_runtime.h>

#include "nb_glm_kernels.hpp"

namespace pilot {

constexpr int NB_DESIGN_MAX_COLS = 8;
constexpr int NB_DESIGN_MAX_ITERS = 100;
constexpr int NB_DESIGN_MAX_HALVINGS = 30;
constexpr double NB_DESIGN_TOL = 1e-10;
constexpr double NB_DESIGN_RIDGE = 1e-6;
constexpr int NB_DESIGN_LDS_BYTES = 96 * 1024;          // of the CU's 160 KiB, as K22's limit

// pilot_ot_nb_design_max_samples: 8 m (2 + p) bytes of LDS, and never more than K22 takes
__host__ __device__ constexpr int nb_design_max_samples(int p) {
    return NB_DESIGN_LDS_BYTES / (8 * (2 + p)) < NB_MAX_SAMPLES ? NB_DESIGN_LDS_BYTES / (8 * (2 + p)) : NB_MAX_SAMPLES;
}

// the packed upper triangle of a symmetric or upper-triangular P x P matrix: (i, j), i <= j
template <int P> __host__ __device__ constexpr int nb_tri(int i, int j) { return i * P - i * (i - 1) / 2 + (j - i); }
template <int P> constexpr int NB_TRI = P * (P + 1) / 2;

// A = U^T U in place (A packed upper, positive definite): U upper triangular
template <int P> __device__ inline void nb_cholesky(double (&A)[NB_TRI<P>]) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
        double d = A[nb_tri<P>(j, j)];
#pragma unroll
        for (int k = 0; k < P; ++k)
            if (k < j) d = fma(-A[nb_tri<P>(k < j ? k : 0, j)], A[nb_tri<P>(k < j ? k : 0, j)], d);
        const double u = sqrt(d), inv = 1.0 / u;
        A[nb_tri<P>(j, j)] = u;
#pragma unroll
        for (int i = 0; i < P; ++i)
            if (i > j) {
                const int ii = i > j ? i : j;
                double v = A[nb_tri<P>(j, ii)];
#pragma unroll
                for (int k = 0; k < P; ++k)
                    if (k < j) v = fma(-A[nb_tri<P>(k < j ? k : 0, j)], A[nb_tri<P>(k < j ? k : 0, ii)], v);
                A[nb_tri<P>(j, ii)] = v * inv;
            }
    }
}

// d with U^T U d = g
template <int P> __device__ inline void nb_cholesky_solve(const double (&U)[NB_TRI<P>], const double (&g)[P], double (&d)[P]) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double v = g[i];
#pragma unroll
        for (int k = 0; k < P; ++k)
            if (k < i) v = fma(-U[nb_tri<P>(k < i ? k : 0, i)], d[k], v);
        d[i] = v / U[nb_tri<P>(i, i)];
    }
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int i = P - 1 - r;
        double v = d[i];
#pragma unroll
        for (int k = 0; k < P; ++k)
            if (k > i) v = fma(-U[nb_tri<P>(i, k > i ? k : i)], d[k], v);
        d[i] = v / U[nb_tri<P>(i, i)];
    }
}

// sum of log U_kk: half the log determinant of U^T U
template <int P> __device__ inline double nb_cholesky_half_logdet(const double (&U)[NB_TRI<P>]) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) s += log(U[nb_tri<P>(k, k)]);
    return s;
}

// S = (U^T U)^-1 = V V^T with V = U^-1, packed upper
template <int P> __device__ inline void nb_cholesky_inverse(const double (&U)[NB_TRI<P>], double (&S)[NB_TRI<P>]) {
    double V[NB_TRI<P>];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double inv = 1.0 / U[nb_tri<P>(j, j)];
        V[nb_tri<P>(j, j)] = inv;
#pragma unroll
        for (int i = 0; i < P; ++i)
            if (i < j) {
                const int ii = i < j ? i : j;
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < P; ++k)
                    if (k >= ii && k < j) v = fma(V[nb_tri<P>(ii, k >= ii ? k : ii)], U[nb_tri<P>(k < j ? k : 0, j)], v);
                V[nb_tri<P>(ii, j)] = -v * inv;
            }
    }
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j)
            if (j >= i) {
                const int jj = j >= i ? j : i;
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < P; ++k)
                    if (k >= jj) v = fma(V[nb_tri<P>(i, k >= jj ? k : jj)], V[nb_tri<P>(jj, k >= jj ? k : jj)], v);
                S[nb_tri<P>(i, jj)] = v;
            }
}

// eta = x^T beta + log s
template <int P> __device__ inline double nb_design_eta(const double (&x)[P], const double (&beta)[P], double ls) {
    double eta = ls;
#pragma unroll
    for (int k = 0; k < P; ++k) eta = fma(x[k], beta[k], eta);
    return eta;
}

// M += w x x^T (packed upper)
template <int P> __device__ inline void nb_design_rank1(double (&M)[NB_TRI<P>], const double (&x)[P], double w) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const double wx = w * x[k];
#pragma unroll
        for (int l = 0; l < P; ++l)
            if (l >= k) M[nb_tri<P>(k, l >= k ? l : k)] = fma(wx, x[l], M[nb_tri<P>(k, l >= k ? l : k)]);
    }
}

// The inner fit from `beta` (in: the start, out: the maximiser).  sample(j, c, ls, x): the count, log size factor and design row of
// sample j.  lambda: the ridge on every coefficient (K26: NB_DESIGN_RIDGE; K27: 1 / sigma0^2, the normal prior of the coefficients
// that are not shrunk).  Returns the Newton steps taken; converged = false after NB_DESIGN_MAX_ITERS of them.
template <int P, typename Sample>
__device__ inline int nb_design_solve(int m, double alpha, double lambda, double (&beta)[P], bool &converged, Sample sample) {
    const double inv_alpha = 1.0 / alpha;
    converged = false;
    int it = 0;
    while (it < NB_DESIGN_MAX_ITERS) {
        ++it;
        double g[P], H[NB_TRI<P>], d[P];
#pragma unroll
        for (int k = 0; k < P; ++k) g[k] = -lambda * beta[k];
#pragma unroll
        for (int t = 0; t < NB_TRI<P>; ++t) H[t] = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) H[nb_tri<P>(k, k)] = lambda;
        for (int j = 0; j < m; ++j) {
            double c, ls, x[P];
            sample(j, c, ls, x);
            const double mu = exp(nb_design_eta<P>(x, beta, ls)), inv = 1.0 / (1.0 + alpha * mu), r = (c - mu) * inv;
            const double w = (mu * inv) * ((1.0 + alpha * c) * inv);     // (in two factors, as K24: (1 + a mu)^2 could overflow)
#pragma unroll
            for (int k = 0; k < P; ++k) g[k] = fma(x[k], r, g[k]);
            nb_design_rank1<P>(H, x, w);
        }
        nb_cholesky<P>(H);
        nb_cholesky_solve<P>(H, g, d);
        double moved = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) moved = fabs(d[k]) > moved ? fabs(d[k]) : moved;
        double t = 1.0;
        // (a whole step within the tolerance is taken unsearched: the change of l is below its own rounding there)
        for (int halvings = 0; !(moved <= NB_DESIGN_TOL) && halvings < NB_DESIGN_MAX_HALVINGS; ++halvings) {
            double change = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) change -= 0.5 * lambda * (t * d[k]) * (2.0 * beta[k] + t * d[k]);
            for (int j = 0; j < m; ++j) {
                double c, ls, x[P];
                sample(j, c, ls, x);
                const double amu = alpha * exp(nb_design_eta<P>(x, beta, ls)), rho = amu / (1.0 + amu);
                double D = 0.0;
#pragma unroll
                for (int k = 0; k < P; ++k) D = fma(x[k], d[k], D);
                D *= t;
                change += c * D - (c + inv_alpha) * log1p(rho * expm1(D));
            }
            if (__builtin_isfinite(change) && change >= 0.0) break;
            t *= 0.5;
        }
#pragma unroll
        for (int k = 0; k < P; ++k) beta[k] = fma(t, d[k], beta[k]);
        if (t * moved <= NB_DESIGN_TOL) { converged = true; break; }      // (t is a power of two; a NaN never stops)
    }
    return it;
}

// the start of a cold fit: (log max(mean_j c_j / s_j, minmu), 0, ...), the mean summed in sample order by the one thread
template <int P, typename Sample> __device__ inline void nb_design_start(int m, const double *__restrict__ s, double (&beta)[P], Sample sample) {
    double sum = 0.0;
    for (int j = 0; j < m; ++j) {
        double c, ls, x[P];
        sample(j, c, ls, x);
        sum += c / s[j];
    }
    const double mean = sum / (double)m;
#pragma unroll
    for (int k = 0; k < P; ++k) beta[k] = 0.0;
    beta[0] = log(mean > NB_MIN_MU ? mean : NB_MIN_MU);
}

// Grid: n_genes workgroups of one wave.  Dynamic LDS: m (2 + P) doubles.  sf: the m size factors, then their m logarithms, then X
// (m x P, row-major).  log_prior_mean: nullable (no prior term).  beta_out: nullable, n_genes x P, the coefficients at the winner.
// steps_out: the Newton steps of all grid points and rounds; flags_out: NB_FLAG_NOT_CONVERGED if any inner fit did not converge.
// A gene of zeros, or one whose prior mean is not finite, gets NaN in log_disp, objective and beta_out (steps = flags = 0).
template <typename T, int P>
__global__ void __launch_bounds__(64) nb_design_dispersion_kernel(const T *__restrict__ Y, long long ld, int m, const double *__restrict__ sf,
                                                                   const double *__restrict__ log_prior_mean, double prior_var,
                                                                   double *__restrict__ log_disp, double *__restrict__ objective,
                                                                   double *__restrict__ beta_out, int *__restrict__ steps_out,
                                                                   int *__restrict__ flags_out) {
    extern __shared__ double nb_design_lds[];
    double *sc = nb_design_lds, *sl = sc + m, *sx = sl + m;
    const int gene = blockIdx.x, lane = threadIdx.x;

    int any = 0;
    for (int j = lane; j < m; j += 64) {
        const double c = rint((double)Y[(long long)j * ld + gene]);
        sc[j] = c;
        sl[j] = sf[m + j];
        any |= c > 0.0;
    }
    for (int t = lane; t < m * P; t += 64) sx[t] = sf[2 * m + t];
    any = lanes_reduce(any, Max{});
    __syncthreads();

    const double lpm = log_prior_mean ? log_prior_mean[gene] : 0.0;
    if (!any || !__builtin_isfinite(lpm)) {
        if (lane == 0) {
            log_disp[gene] = objective[gene] = __builtin_nan("");
            steps_out[gene] = flags_out[gene] = 0;
        }
        if (beta_out && lane < P) beta_out[(long long)gene * P + lane] = __builtin_nan("");
        return;
    }
    const auto sample = [&](int j, double &c, double &ls, double (&x)[P]) {
        c = sc[j];
        ls = sl[j];
#pragma unroll
        for (int k = 0; k < P; ++k) x[k] = sx[j * P + k];
    };
    const double half_inv_var = log_prior_mean ? 0.5 / prior_var : 0.0;
    double start[P], beta[P];
    nb_design_start<P>(m, sf, start, sample);
    double x = 0.0, L = 0.0;
    int steps = 0, flags = 0;
    nb_grid_rounds(log(NB_MIN_DISP), log(nb_max_disp(m)), lane, [&](int, double at) {
        x = at;
        const double alpha = exp(x), r = 1.0 / alpha, lg_r = lgamma(r);
#pragma unroll
        for (int k = 0; k < P; ++k) beta[k] = start[k];
        bool done;
        steps += nb_design_solve<P>(m, alpha, NB_DESIGN_RIDGE, beta, done, sample);
        if (!done) flags |= NB_FLAG_NOT_CONVERGED;
        double M[NB_TRI<P>];
#pragma unroll
        for (int t = 0; t < NB_TRI<P>; ++t) M[t] = 0.0;
        L = 0.0;
        for (int j = 0; j < m; ++j) {
            double c, ls, xr[P];
            sample(j, c, ls, xr);
            double mu = exp(nb_design_eta<P>(xr, beta, ls));
            mu = mu > NB_MIN_MU ? mu : NB_MIN_MU;
            const double am = alpha * mu, l1p = log1p(am);
            if (c > 0.0) L += lgamma(c + r) - lg_r - (c + r) * l1p + c * log(am);
            else L -= r * l1p;
            nb_design_rank1<P>(M, xr, mu / (1.0 + am));
        }
        nb_cholesky<P>(M);
        L -= nb_cholesky_half_logdet<P>(M);
        if (log_prior_mean) L -= (x - lpm) * (x - lpm) * half_inv_var;
        return L;
    }, [&](int round, int b) {
#pragma unroll
        for (int k = 0; k < P; ++k) start[k] = __shfl(beta[k], b, 64);
        if (round == NB_ROUNDS - 1) {
            const int total = lanes_reduce(steps, Sum{}), all = lanes_reduce(flags, Max{});
            if (lane == b) {
                log_disp[gene] = x;
                objective[gene] = L;
                steps_out[gene] = total;
                flags_out[gene] = all;
                if (beta_out) {
#pragma unroll
                    for (int k = 0; k < P; ++k) beta_out[(long long)gene * P + k] = beta[k];
                }
            }
        }
    });
}

// Grid: ceil(n_genes / 256) workgroups; thread t: gene t.  sf as above.  beta: n_genes x P; cov: n_genes x P (P + 1) / 2, the packed
// upper triangle of Sigma.  A NaN dispersion or a gene of zeros leaves its gene out (NaN everywhere, steps = flags = 0).
template <typename T, int P>
__global__ void __launch_bounds__(256) nb_design_fit_kernel(const T *__restrict__ Y, long long ld, int m, int n_genes,
                                                             const double *__restrict__ sf, const double *__restrict__ dispersion,
                                                             double *__restrict__ beta_out, double *__restrict__ cov_out,
                                                             double *__restrict__ loglik_out, int *__restrict__ steps_out,
                                                             int *__restrict__ flags_out) {
    const int gene = blockIdx.x * blockDim.x + threadIdx.x;
    if (gene >= n_genes) return;
    const double *sl = sf + m, *X = sf + 2 * m;
    const double alpha = dispersion[gene];
    const auto sample = [&](int j, double &c, double &ls, double (&x)[P]) {
        c = rint((double)Y[(long long)j * ld + gene]);
        ls = sl[j];
#pragma unroll
        for (int k = 0; k < P; ++k) x[k] = X[j * P + k];
    };
    double beta[P], S[NB_TRI<P>];
    int any = 0;
    for (int j = 0; j < m; ++j) any |= rint((double)Y[(long long)j * ld + gene]) > 0.0;
    if (alpha != alpha || !any) {
#pragma unroll
        for (int k = 0; k < P; ++k) beta_out[(long long)gene * P + k] = __builtin_nan("");
#pragma unroll
        for (int t = 0; t < NB_TRI<P>; ++t) cov_out[(long long)gene * NB_TRI<P> + t] = __builtin_nan("");
        loglik_out[gene] = __builtin_nan("");
        steps_out[gene] = flags_out[gene] = 0;
        return;
    }
    nb_design_start<P>(m, sf, beta, sample);
    bool done;
    const int steps = nb_design_solve<P>(m, alpha, NB_DESIGN_RIDGE, beta, done, sample);

    const double r = 1.0 / alpha, lg_r = lgamma(r);
    double M[NB_TRI<P>], loglik = 0.0;
#pragma unroll
    for (int t = 0; t < NB_TRI<P>; ++t) M[t] = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) M[nb_tri<P>(k, k)] = NB_DESIGN_RIDGE;
    for (int j = 0; j < m; ++j) {
        double c, ls, x[P];
        sample(j, c, ls, x);
        const double mu = exp(nb_design_eta<P>(x, beta, ls)), am = alpha * mu;
        if (c > 0.0) loglik += lgamma(c + r) - lg_r - lgamma(c + 1.0) - (c + r) * log1p(am) + c * log(am);
        else loglik -= r * log1p(am);
        const double fl = mu > NB_MIN_MU ? mu : NB_MIN_MU;
        nb_design_rank1<P>(M, x, fl / (1.0 + alpha * fl));
    }
    nb_cholesky<P>(M);
    nb_cholesky_inverse<P>(M, S);
#pragma unroll
    for (int k = 0; k < P; ++k) beta_out[(long long)gene * P + k] = beta[k];
#pragma unroll
    for (int t = 0; t < NB_TRI<P>; ++t) cov_out[(long long)gene * NB_TRI<P> + t] = S[t];
    loglik_out[gene] = loglik;
    steps_out[gene] = steps;
    flags_out[gene] = done ? 0 : NB_FLAG_NOT_CONVERGED;
}

}  // namespace pilot
