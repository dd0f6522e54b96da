// K9: trajectory model fits (pilotpy's fit_best_model / fit_model_activity, the engine behind cell_importance and
// genes_importance).  For every target column y of a dense n x T observations matrix and the shared time vector x, three
// models with an intercept -- linear [x], linear_quadratic [x, x^2], quadratic [x^2] -- fitted by OLS or to the optimum of
// scikit-learn's HuberRegressor objective (concomitant scale), then R^2, the modified R^2, t-test p-values of the
// coefficients, the model choice, slope, pattern and the Pearson test.
//
// Layout: one lane per target; a workgroup owns 64 adjacent targets and its TF_WAVES waves split the observations into fixed
// slices.  Per-wave partial sums meet in LDS and every wave adds them in wave order, so every wave holds the same totals
// and a call is bit-reproducible (no value atomics).  All arithmetic is f64 whatever the input type.
//
// Conditioning: the kernel never touches the raw powers of x.  The host maps x to u = (x - m) / s (m = mean(x),
// s = max |x - m|, so |u| <= 1) and passes, per model, the 3 x 3 matrices that turn the moments M = (sum y, sum u y,
// sum u^2 y) into the fit in a well-conditioned basis (G), its prediction polynomial in u (C), the coefficients in the
// original basis (R) and diag((Z^T Z)^-1) (vd), all formed on the host from the 3 x 3 Gram of [1, u, u^2].
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "reduce.hpp"

namespace pilot {

constexpr int TF_WAVES = 8;                       // waves of a workgroup: observation slices
constexpr int TF_BLOCK = 64 * TF_WAVES;
constexpr int TF_NACC = 15;                       // LDS partials per lane and wave (the Huber pass has 15)
constexpr int TF_NOUT = 40;                       // doubles per target in the output record (layout: TF_O_*)
constexpr int TF_O_PARAMS = 0, TF_O_PVAL = 9, TF_O_R2 = 18, TF_O_MR2 = 21, TF_O_SIGMA = 24, TF_O_STEPS = 27, TF_O_FLAGS = 30,
              TF_O_CHOSEN = 33, TF_O_SLOPE = 34, TF_O_PATTERN = 35, TF_O_PR = 36, TF_O_PP = 37, TF_O_ZERO = 38, TF_O_MEAN = 39;
constexpr int TF_FLAG_NOT_CONVERGED = 1;
constexpr double TF_HUBER_TOL = 1e-12;            // optimality: (sum |projected gradient|) * sigma <= TF_HUBER_TOL * objective
constexpr int TF_LS_EVALS = 60;                   // objective evaluations of one line search

struct TrajfitModel {
    double G[3][3];    // gamma = G M: fit coefficients in the model's scaled basis b(u) (p entries used)
    double C[3][3];    // delta = C gamma: prediction y_hat(u) = delta0 + delta1 u + delta2 u^2
    double R[3][3];    // beta = R gamma: coefficients on [1, f(x)]
    double pen[3][3];  // alpha ||w||^2 written on gamma (w = the non-intercept part of beta)
    double vd[3];      // diag((Z^T Z)^-1), Z = [1, f(x)]
};

struct TrajfitArgs {
    TrajfitModel mod[3];           // linear, linear_quadratic, quadratic
    double quad_k;                 // quadratic basis column b1 = (u^2 + quad_k u) * quad_scale
    double quad_scale;
    double sxx;                    // sum (u - mean u)^2 (Pearson)
    double x_min, x_max;
    double epsilon, pval_thr, sigma_min;
    int n, huber, modify_r2, max_iter;
};

// number of coefficients (intercept included) of model m
__device__ __forceinline__ int tf_p(int m) { return m == 1 ? 3 : 2; }

// the model's basis vector b(u) (p entries): delta = C gamma means b = C^T [1, u, u^2]
__device__ __forceinline__ void tf_basis(const TrajfitArgs &a, int m, double u, double b[3]) {
    b[0] = 1.0;
    if (m == 0) { b[1] = u; b[2] = 0.0; }
    else if (m == 1) { b[1] = u; b[2] = u * u; }
    else { b[1] = (u * u + a.quad_k * u) * a.quad_scale; b[2] = 0.0; }
}

// ln(Gamma(a + 1/2) / Gamma(a)), a > 0: lgamma below 16; above, Stirling's series written so that nothing cancels
// (a ln(a + 1/2) - (a - 1/2) ln a = a log1p(1 / (2a)) + ln(a) / 2)
__device__ inline double tf_lgamma_ratio_half(double a) {
    if (a < 16.0) return lgamma(a + 0.5) - lgamma(a);
    auto corr = [](double z) {
        const double iz = 1.0 / z, iz2 = iz * iz;
        return iz * (1.0 / 12.0 - iz2 * (1.0 / 360.0 - iz2 * (1.0 / 1260.0 - iz2 * (1.0 / 1680.0))));
    };
    return a * log1p(0.5 / a) + 0.5 * log(a) - 0.5 + (corr(a + 0.5) - corr(a));
}

// continued fraction of the incomplete beta (modified Lentz), converges for x < (a + 1) / (a + b + 2)
__device__ inline double tf_betacf(double a, double b, double x) {
    const double FPMIN = 1e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < FPMIN) d = FPMIN;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 100000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (fabs(d) < FPMIN) d = FPMIN;
        c = 1.0 + aa / c; if (fabs(c) < FPMIN) c = FPMIN;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (fabs(d) < FPMIN) d = FPMIN;
        c = 1.0 + aa / c; if (fabs(c) < FPMIN) c = FPMIN;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= 1e-16) break;
    }
    return h;
}

// regularised incomplete beta I_x(a, 1/2), given x and y = 1 - x (each accurate on its own)
__device__ inline double tf_ibeta_half(double a, double x, double y) {
    if (!(x > 0.0)) return x == 0.0 ? 0.0 : NAN;
    if (!(y > 0.0)) return y == 0.0 ? 1.0 : NAN;
    const double b = 0.5;
    const double ln_front = a * log(x) + b * log(y) + tf_lgamma_ratio_half(a) - 0.5723649429247001;   // - ln Gamma(1/2)
    const double front = exp(ln_front);
    if (x < (a + 1.0) / (a + b + 2.0)) return front * tf_betacf(a, b, x) / a;
    return 1.0 - front * tf_betacf(b, a, y) / b;
}

// two-sided t-test p-value 2 (1 - Tcdf(|t|, nu)), written as one minus the CDF like the reference
__device__ inline double tf_t_pvalue(double t, double nu) {
    if (isnan(t)) return NAN;
    const double t2 = t * t;
    double cdf;
    if (isinf(t2)) cdf = 1.0;
    else {
        const double den = nu + t2;
        cdf = 1.0 - 0.5 * tf_ibeta_half(0.5 * nu, nu / den, t2 / den);
    }
    return 2.0 * (1.0 - cdf);
}

// all waves add the TF_WAVES partials of `cnt` accumulators in wave order (every wave gets the same totals)
__device__ __forceinline__ void tf_reduce(double (*lds)[TF_NACC][64], const double *part, double *tot, int cnt, int wave, int lane) {
    for (int k = 0; k < cnt; ++k) lds[wave][k][lane] = part[k];
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
        double s = 0.0;
        for (int w = 0; w < TF_WAVES; ++w) s += lds[w][k][lane];
        tot[k] = s;
    }
    __syncthreads();
}

// Solve (H + ridge I) z = r (k <= 4) by Cholesky, the ridge 1e-10 max|diag H| and grown tenfold while the factorisation fails
__device__ inline void tf_spd_solve(const double H[4][4], const double *r, double *z, int k) {
    double L[4][4] = {};
    double dmax = 0.0;
    for (int i = 0; i < k; ++i) dmax = fmax(dmax, fabs(H[i][i]));
    if (!(dmax > 0.0)) dmax = 1.0;
    double ridge = 1e-10 * dmax;
    for (int attempt = 0; attempt < 40; ++attempt) {
        bool ok = true;
        for (int i = 0; i < k && ok; ++i) {
            for (int j = 0; j <= i; ++j) {
                double s = H[i][j] + (i == j ? ridge : 0.0);
                for (int l = 0; l < j; ++l) s -= L[i][l] * L[j][l];
                if (i == j) {
                    if (!(s > 0.0)) { ok = false; break; }
                    L[i][i] = sqrt(s);
                } else {
                    L[i][j] = s / L[j][j];
                }
            }
        }
        if (ok) break;
        ridge *= 10.0;
    }
    double w[4];
    for (int i = 0; i < k; ++i) {
        double s = r[i];
        for (int l = 0; l < i; ++l) s -= L[i][l] * w[l];
        w[i] = s / L[i][i];
    }
    for (int i = k - 1; i >= 0; --i) {
        double s = w[i];
        for (int l = i + 1; l < k; ++l) s -= L[l][i] * z[l];
        z[i] = s / L[i][i];
    }
}

// Huber objective F, gradient g and Hessian H over (gamma_0 .. gamma_{p-1}, sigma) from the pass sums S:
// [0] sum r^2 (inliers), [1..3] sum r b (inliers), [4..9] sum b b^T (inliers, packed 00 01 02 11 12 22),
// [10] sum |r| (outliers), [11..13] sum sign(r) b (outliers), [14] outlier count
__device__ inline void tf_huber_eval(const TrajfitArgs &a, int m, const double *gam, double sigma, const double *S, double &F,
                                     double g[4], double H[4][4]) {
    const int p = tf_p(m);
    const double n = a.n, eps = a.epsilon;
    const int pk[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
    double pen_g[3] = {0.0, 0.0, 0.0}, pen = 0.0;
    for (int i = 0; i < p; ++i) {
        for (int j = 0; j < p; ++j) pen_g[i] += a.mod[m].pen[i][j] * gam[j];
        pen += gam[i] * pen_g[i];
    }
    F = n * sigma + S[0] / sigma + 2.0 * eps * S[10] - eps * eps * sigma * S[14] + pen;
    for (int i = 0; i < 4; ++i) {
        g[i] = 0.0;
        for (int j = 0; j < 4; ++j) H[i][j] = 0.0;
    }
    for (int i = 0; i < p; ++i) g[i] = -2.0 * S[1 + i] / sigma - 2.0 * eps * S[11 + i] + 2.0 * pen_g[i];
    g[p] = n - S[0] / (sigma * sigma) - eps * eps * S[14];
    for (int i = 0; i < p; ++i) {
        for (int j = 0; j < p; ++j) H[i][j] = 2.0 * S[pk[i][j]] / sigma + 2.0 * a.mod[m].pen[i][j];
        H[i][p] = H[p][i] = 2.0 * S[1 + i] / (sigma * sigma);
    }
    H[p][p] = 2.0 * S[0] / (sigma * sigma * sigma);
}

// One kernel per chunk of targets.  Y: n rows of `ld` elements (the chunk's first target at column 0), T = float or double.
// out: TF_NOUT doubles per target of the chunk.
template <typename T>
__global__ void __launch_bounds__(TF_BLOCK) trajfit_kernel(const T *__restrict__ Y, long long ld, int n_targets,
                                                           const double *__restrict__ u, const TrajfitArgs *__restrict__ args,
                                                           double *__restrict__ out) {
    const TrajfitArgs &a = *args;             // (in global memory: indexed by model, the struct would be copied to scratch)
    __shared__ double lds[TF_WAVES][TF_NACC][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane;
    const bool valid = t < n_targets;
    const int n = a.n;
    const long long i0 = (long long)n * wave / TF_WAVES, i1 = (long long)n * (wave + 1) / TF_WAVES;
    const T *col = Y + (valid ? t : 0);
    auto yat = [&](long long i) -> double { return valid ? (double)col[i * ld] : 0.0; };

    // pass 1: moments, sum y^2, zeros, values different from the first
    double part[TF_NACC], tot[TF_NACC];
    {
        const double y0 = yat(0);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, syy = 0.0, nz = 0.0, nd = 0.0;
#pragma unroll 8
        for (long long i = i0; i < i1; ++i) {
            const double y = yat(i), ui = u[i];
            s0 += y;
            s1 += ui * y;
            s2 += ui * ui * y;
            syy += y * y;
            nz += y == 0.0 ? 1.0 : 0.0;
            nd += y != y0 ? 1.0 : 0.0;
        }
        part[0] = s0; part[1] = s1; part[2] = s2; part[3] = syy; part[4] = nz; part[5] = nd;
        tf_reduce(lds, part, tot, 6, wave, lane);
    }
    const double M[3] = {tot[0], tot[1], tot[2]};
    const double syy = tot[3], zeros = tot[4];
    const bool constant = tot[5] == 0.0;

    // OLS fits: gamma = G M
    double gam[3][3];
    for (int m = 0; m < 3; ++m)
        for (int i = 0; i < 3; ++i) gam[m][i] = a.mod[m].G[i][0] * M[0] + a.mod[m].G[i][1] * M[1] + a.mod[m].G[i][2] * M[2];
    double sig[3] = {NAN, NAN, NAN};
    int steps[3] = {0, 0, 0}, flags[3] = {0, 0, 0};
    if (a.huber) {
        // Newton steps on (gamma, sigma) with a bracketing line search on the directional derivative (the objective is convex
        // along any line; where most points are outliers it is nearly linear along a joint scaling of (gamma, sigma), which a
        // fixed-step Newton overshoots).  Every wave holds identical lane states, so the loop condition is workgroup-uniform.
        for (int m = 0; m < 3; ++m) {
            const int p = tf_p(m), k = p + 1;
            double cg[3] = {gam[m][0], gam[m][1], gam[m][2]}, cs;
            bool done = !valid;
            if (constant) {                           // the optimum: the constant itself, sigma at its bound
                cg[0] = yat(0); cg[1] = 0.0; cg[2] = 0.0;
                cs = a.sigma_min;
                done = true;
            } else {                                  // start: the OLS fit, sigma = its rms residual
                double proj = 0.0;                    // gamma^T B^T y = sum y_hat^2, B^T y = C^T M
                for (int i = 0; i < p; ++i) proj += cg[i] * (a.mod[m].C[0][i] * M[0] + a.mod[m].C[1][i] * M[1] + a.mod[m].C[2][i] * M[2]);
                const double sse = syy - proj;
                cs = fmax(sse > 1e-8 * syy ? sqrt(sse / n) : sqrt(syy / n), a.sigma_min);
            }
            double cF = 0.0, d[4] = {0.0, 0.0, 0.0, 0.0}, s0 = 0.0, t = 0.0, tmax = 0.0, lo = 0.0, flo = 0.0, hi = -1.0, fhi = 0.0;
            double bt = 0.0, bF = 0.0, bg[4] = {}, bH[4][4] = {};
            bool start = true, have_best = false;
            int it = 0, fl = 0, evals = 0;
            while (__any(!done)) {
                const double es = start ? cs : fmax(cs + t * d[p], a.sigma_min);
                double eg[3];
                for (int i = 0; i < 3; ++i) eg[i] = start ? cg[i] : cg[i] + t * d[i];
                double S[TF_NACC];
                for (int q = 0; q < TF_NACC; ++q) S[q] = 0.0;
                if (!done) {
                    const double thr = a.epsilon * es;
                    for (long long i = i0; i < i1; ++i) {
                        double b[3];
                        tf_basis(a, m, u[i], b);
                        const double r = yat(i) - (eg[0] * b[0] + eg[1] * b[1] + eg[2] * b[2]);
                        if (fabs(r) <= thr) {
                            S[0] += r * r;
                            S[1] += r * b[0]; S[2] += r * b[1]; S[3] += r * b[2];
                            S[4] += b[0] * b[0]; S[5] += b[0] * b[1]; S[6] += b[0] * b[2];
                            S[7] += b[1] * b[1]; S[8] += b[1] * b[2]; S[9] += b[2] * b[2];
                        } else {
                            const double sg = r > 0.0 ? 1.0 : -1.0;
                            S[10] += fabs(r);
                            S[11] += sg * b[0]; S[12] += sg * b[1]; S[13] += sg * b[2];
                            S[14] += 1.0;
                        }
                    }
                }
                double St[TF_NACC];
                tf_reduce(lds, S, St, TF_NACC, wave, lane);
                if (done) continue;
                double F, g[4], H[4][4];
                tf_huber_eval(a, m, eg, es, St, F, g, H);
                bool accept = start;
                if (!start) {                             // line search: bracket the zero of phi'(t) = g . d
                    double st = 0.0;
                    for (int i = 0; i < k; ++i) st += g[i] * d[i];
                    ++evals;
                    if (F <= cF && fabs(st) <= 0.1 * fabs(s0)) {
                        have_best = true; bt = t; bF = F;
                        for (int i = 0; i < 4; ++i) { bg[i] = g[i]; for (int j = 0; j < 4; ++j) bH[i][j] = H[i][j]; }
                    } else {
                        bool finish = evals >= TF_LS_EVALS;
                        if (st < 0.0) {
                            if (F <= cF) {
                                have_best = true; bt = t; bF = F;
                                for (int i = 0; i < 4; ++i) { bg[i] = g[i]; for (int j = 0; j < 4; ++j) bH[i][j] = H[i][j]; }
                            }
                            lo = t; flo = st;
                            if (hi < 0.0) {
                                if (t >= tmax) finish = true;
                                else if (!finish) { t = fmin(4.0 * t, tmax); continue; }
                            }
                        } else {
                            hi = t; fhi = st;
                        }
                        if (!finish) {
                            t = lo + (hi - lo) * fmin(fmax(-flo / (fhi - flo), 0.05), 0.95);
                            continue;
                        }
                        if (!have_best) { done = true; continue; }       // no lower objective in floating point: at the optimum
                    }
                    // accept the best point of the line search
                    for (int i = 0; i < p; ++i) cg[i] += bt * d[i];
                    cs = fmax(cs + bt * d[p], a.sigma_min);
                    F = bF;
                    for (int i = 0; i < 4; ++i) { g[i] = bg[i]; for (int j = 0; j < 4; ++j) H[i][j] = bH[i][j]; }
                    accept = true;
                }
                if (accept) {
                    start = false;
                    cF = F;
                    const bool bound = cs <= a.sigma_min && g[p] > 0.0;     // sigma held at its bound: projected gradient
                    if (bound) {
                        g[p] = 0.0;
                        for (int i = 0; i < k; ++i) H[i][p] = H[p][i] = 0.0;
                        H[p][p] = 1.0;
                    }
                    double gn = 0.0;
                    for (int i = 0; i < k; ++i) gn += fabs(g[i]);
                    if (gn * cs <= TF_HUBER_TOL * fabs(F)) { done = true; continue; }          // the optimality test
                    if (it >= a.max_iter) { done = true; fl = TF_FLAG_NOT_CONVERGED; continue; }
                    ++it;
                    double mg[4];
                    for (int i = 0; i < k; ++i) mg[i] = -g[i];
                    tf_spd_solve(H, mg, d, k);
                    if (bound) d[p] = 0.0;
                    s0 = 0.0;
                    for (int i = 0; i < k; ++i) s0 += g[i] * d[i];
                    if (!(s0 < 0.0)) {                                      // (not a descent direction: steepest descent)
                        for (int i = 0; i < k; ++i) d[i] = -g[i];
                        s0 = 0.0;
                        for (int i = 0; i < k; ++i) s0 -= g[i] * g[i];
                    }
                    for (int i = k; i < 4; ++i) d[i] = 0.0;
                    tmax = d[p] < 0.0 ? (cs - a.sigma_min) / -d[p] : INFINITY;
                    t = fmin(1.0, tmax);
                    lo = 0.0; flo = s0; hi = -1.0; evals = 0; have_best = false;
                }
            }
            for (int i = 0; i < 3; ++i) gam[m][i] = cg[i];
            sig[m] = cs;
            steps[m] = it;
            flags[m] = fl;
        }
    }

    // prediction polynomials in u
    double del[3][3];
    for (int m = 0; m < 3; ++m)
        for (int i = 0; i < 3; ++i) del[m][i] = a.mod[m].C[i][0] * gam[m][0] + a.mod[m].C[i][1] * gam[m][1] + a.mod[m].C[i][2] * gam[m][2];
    const double ybar = M[0] / n;

    // pass 2: residuals -> SSE, the modified SSE, SST, sum u (y - ybar)
    {
        double sse[3] = {0.0, 0.0, 0.0}, msse[3] = {0.0, 0.0, 0.0}, sst = 0.0, sxy = 0.0;
#pragma unroll 4
        for (long long i = i0; i < i1; ++i) {
            const double y = yat(i), ui = u[i];
            for (int m = 0; m < 3; ++m) {
                const double e = y - (del[m][0] + ui * (del[m][1] + ui * del[m][2]));
                sse[m] += e * e;
                const double ae = fabs(e);
                msse[m] += ae < 1.35 ? 0.5 * e * e : 1.35 * (ae - 0.675);
            }
            const double dy = y - ybar;
            sst += dy * dy;
            sxy += ui * dy;
        }
        for (int m = 0; m < 3; ++m) { part[m] = sse[m]; part[3 + m] = msse[m]; }
        part[6] = sst; part[7] = sxy;
        tf_reduce(lds, part, tot, 8, wave, lane);
    }
    if (wave != 0 || !valid) return;

    const double sst = constant ? 0.0 : tot[6];
    double *o = out + (long long)t * TF_NOUT;
    int chosen = -1;
    double best = -1000.0;
    double beta_c[3] = {0.0, 0.0, 0.0};
    for (int m = 0; m < 3; ++m) {
        const int p = tf_p(m), q = p - 1;
        const double sse = tot[m], msse = tot[3 + m];
        double beta[3];
        for (int i = 0; i < 3; ++i) beta[i] = a.mod[m].R[i][0] * gam[m][0] + a.mod[m].R[i][1] * gam[m][1] + a.mod[m].R[i][2] * gam[m][2];
        const double r2 = sst > 0.0 ? 1.0 - sse / sst : (sse == 0.0 ? 1.0 : 0.0);
        const double adj_f = (double)(n - 1) / (double)(n - q - 1);
        const double r2a = 1.0 - (1.0 - r2) * adj_f;
        const double mr2 = 1.0 - msse / sst;
        const double mr2a = 1.0 - (1.0 - mr2) * adj_f;
        const double nu = n - p, mse = sse / nu;
        bool eligible = flags[m] == 0;
        for (int j = 0; j < 3; ++j) {
            double pv = NAN;
            if (j < p) {
                pv = tf_t_pvalue(beta[j] / sqrt(mse * a.mod[m].vd[j]), nu);
                eligible = eligible && pv <= a.pval_thr;
            }
            o[TF_O_PARAMS + 3 * m + j] = j < p ? beta[j] : NAN;
            o[TF_O_PVAL + 3 * m + j] = pv;
        }
        o[TF_O_R2 + m] = r2a;
        o[TF_O_MR2 + m] = mr2a;
        o[TF_O_SIGMA + m] = sig[m];
        o[TF_O_STEPS + m] = steps[m];
        o[TF_O_FLAGS + m] = flags[m];
        const double r2c = a.modify_r2 ? mr2a : r2a;
        if (eligible && r2c > best) {
            best = r2c;
            chosen = m;
            for (int j = 0; j < 3; ++j) beta_c[j] = j < p ? beta[j] : 0.0;
        }
    }
    double slope = NAN, pattern = -1.0;
    if (chosen >= 0) {
        // curve(x) = beta0 + beta1 f1(x) (+ beta2 x^2); the reference's slope is the curve's rise over [x_min, x_max]
        auto curve = [&](double x) {
            if (chosen == 0) return beta_c[0] + beta_c[1] * x;
            if (chosen == 2) return beta_c[0] + beta_c[1] * (x * x);
            return beta_c[0] + beta_c[1] * x + beta_c[2] * (x * x);
        };
        slope = (curve(a.x_max) - curve(a.x_min)) / (a.x_max - a.x_min);
        pattern = (beta_c[1] >= 0.0 ? 0.0 : 1.0) + (chosen == 1 && !(beta_c[2] >= 0.0) ? 2.0 : 0.0);
    }
    o[TF_O_CHOSEN] = chosen;
    o[TF_O_SLOPE] = slope;
    o[TF_O_PATTERN] = pattern;
    double r = NAN, pp = NAN;
    if (!constant) {
        r = tot[7] / sqrt(a.sxx * sst);
        r = fmax(fmin(r, 1.0), -1.0);
        const double ar = fabs(r);
        pp = tf_ibeta_half(0.5 * (n - 2), (1.0 - ar) * (1.0 + ar), r * r);
    }
    o[TF_O_PR] = r;
    o[TF_O_PP] = pp;
    o[TF_O_ZERO] = zeros / n;
    o[TF_O_MEAN] = M[0] / n;
}

// genes_importance's optional scanpy step, normalize_total(target_sum) then log1p, for the chosen columns of one row per
// workgroup: the row's total over ALL columns in f64 (strided per-thread partials, then a fixed LDS tree), out[j] =
// log1p(X[cols[j]] * target_sum / total) (a row without counts stays 0).
constexpr int TF_NORM_THREADS = 256;

template <typename T>
__global__ void __launch_bounds__(TF_NORM_THREADS) trajfit_normalize_kernel(const T *__restrict__ X, int n_genes, const int *__restrict__ cols,
                                                                            int n_cols, double target_sum, T *__restrict__ out) {
    __shared__ double red[TF_NORM_THREADS];
    const T *row = X + (long long)blockIdx.x * n_genes;
    double s = 0.0;
    for (int j = threadIdx.x; j < n_genes; j += TF_NORM_THREADS) s += (double)row[j];
    red[threadIdx.x] = s;
    __syncthreads();
    tree_fold<TF_NORM_THREADS>(red, Sum{});
    const double total = red[0];
    const double scale = total > 0.0 ? target_sum / total : 0.0;
    T *o = out + (long long)blockIdx.x * n_cols;
    for (int j = threadIdx.x; j < n_cols; j += TF_NORM_THREADS) o[j] = (T)log1p((double)row[cols[j]] * scale);
}

}  // namespace pilot
