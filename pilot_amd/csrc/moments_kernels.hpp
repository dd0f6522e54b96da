// K12: per-group count, mean and centred sum of squares of every selected column of a cells x genes matrix -- the quantities
// limma's two-group fit, scanpy's dispersion statistics (of expm1(X)) and Welch's t all follow from (tl.compute_diff_expressions,
// tl.highly_variable_genes, tl.cell_type_diff_two_sub_patient_groups).  One pass over Y from HBM, f64 throughout.
//
// Grid (column tiles of GM_TILE, row slices), one wave per workgroup.  A lane owns GM_V consecutive columns, so a wave reads
// GM_TILE consecutive elements of a row, 16 bytes per lane per load where the layout allows it.  A row's group code is the same
// for every lane: it is read once per row through a wave-uniform address.  The wave walks its slice in chunks of GM_R rows held
// in registers (GM_R loads in flight per lane), and per chunk and group takes the chunk's sum, its mean, and the squared
// deviations from that mean -- two passes over registers, not over memory -- and joins them to the running (count, mean, m2)
// by Chan's update
//     delta = mean_c - mean;  mean += delta * n_c / (n + n_c);  m2 += m2_c + delta^2 * n * n_c / (n + n_c).
// The counts are wave-uniform, so the two weights cost one division each per chunk and group, not per column.  Every value is
// taken relative to a per-slice, per-column shift (the transformed value of the slice's first USED row, code >= 0, when finite,
// else 0; a skipped row never sets it), which keeps the running means small beside the spread when mean / std is large and the
// groups of the call lie within a few spreads of each other; the shift goes back into the slice's mean at the end.  No raw
// sum(y^2) - n mean^2 is formed anywhere.  A second kernel joins the slice partials by the same update IN SLICE ORDER, one
// thread per (group, column): no atomics, the same bits on every run and whatever the route Y came by.
#pragma once
#include <hip/hip_runtime.h>

namespace pilot {

constexpr int GM_V = 4;                 // columns per lane
constexpr int GM_TILE = 64 * GM_V;      // columns per wave
constexpr int GM_R = 8;                 // rows per register chunk
constexpr int GM_MAX_GROUPS = 8;
constexpr int GM_MIN_SLICE_ROWS = 128;  // the host makes n / 128 slices at most, so each has at least this many rows (or all n)

__device__ inline void gm_load4(const float *p, float (&o)[GM_V]) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ inline void gm_load4(const double *p, double (&o)[GM_V]) {
    const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
}

// Y: row-major, leading dimension ld.  codes: n ints, < 0 = row skipped, otherwise < NG.  cols (nullable): the selected columns.
// vec: rows may be read 16 bytes at a time (no cols, ld and the base address multiples of 16 bytes).  Partials, slice-major:
// pcount[slice][NG], pmean / pm2[slice][NG][n_sel].  A (slice, group) without rows leaves count 0 and unspecified mean / m2.
template <typename T, int NG, bool EXPM1>
__global__ void __launch_bounds__(64) group_moments_kernel(const T *__restrict__ Y, long long ld, long long n,
                                                           const int *__restrict__ codes, const int *__restrict__ cols, int n_sel,
                                                           int vec, long long *__restrict__ pcount, double *__restrict__ pmean,
                                                           double *__restrict__ pm2) {
    const int lane = threadIdx.x, slice = blockIdx.y, n_slices = gridDim.y;
    const int j0 = blockIdx.x * GM_TILE + lane * GM_V;
    const long long i0 = n / n_slices * slice + n % n_slices * slice / n_slices;
    const long long i1 = n / n_slices * (slice + 1) + n % n_slices * (slice + 1) / n_slices;
    const bool wide = vec && j0 + GM_V <= n_sel;
    long long cj[GM_V];                                    // this lane's columns; those past the end repeat the last one
#pragma unroll
    for (int v = 0; v < GM_V; ++v) {
        const int j = min(j0 + v, n_sel - 1);
        cj[v] = cols ? cols[j] : j;
    }
    auto load_row = [&](long long i, T (&o)[GM_V]) {
        const T *row = Y + i * ld;
        if (wide) gm_load4(row + j0, o);
        else {
#pragma unroll
            for (int v = 0; v < GM_V; ++v) o[v] = row[cj[v]];
        }
    };
    auto value = [](T y) { return EXPM1 ? expm1((double)y) : (double)y; };

    double shift[GM_V] = {}, mean[NG][GM_V] = {}, m2[NG][GM_V] = {};
    long long cnt[NG] = {};
    // The shift comes from the slice's first USED row: a skipped row's values may lie on another scale altogether, and as the
    // origin of every d they would cost the digits the shift is there to keep.  The codes are wave-uniform, so this is a scalar
    // walk, GM_R codes per step, that never touches Y; a slice without a used row keeps shift 0 and every count 0.
    long long ik = i1;
    for (long long ib = i0; ib < i1 && ik == i1; ib += GM_R) {
        int c[GM_R];
#pragma unroll
        for (int r = 0; r < GM_R; ++r) c[r] = ib + r < i1 ? __builtin_amdgcn_readfirstlane(codes[ib + r]) : -1;
#pragma unroll
        for (int r = GM_R - 1; r >= 0; --r)
            if (c[r] >= 0) ik = ib + r;
    }
    if (ik < i1) {
        T first[GM_V];
        load_row(ik, first);
#pragma unroll
        for (int v = 0; v < GM_V; ++v) {
            const double k = value(first[v]);
            shift[v] = isfinite(k) ? k : 0.0;
        }
    }
    for (long long ib = i0; ib < i1; ib += GM_R) {
        int c[GM_R];
        T raw[GM_R][GM_V];
#pragma unroll
        for (int r = 0; r < GM_R; ++r) {                   // every load of the chunk is issued before the first use
            const bool in = ib + r < i1;
            const long long i = in ? ib + r : i1 - 1;
            c[r] = in ? __builtin_amdgcn_readfirstlane(codes[i]) : -1;
            load_row(i, raw[r]);
        }
        double d[GM_R][GM_V];
#pragma unroll
        for (int r = 0; r < GM_R; ++r)
#pragma unroll
            for (int v = 0; v < GM_V; ++v) d[r][v] = value(raw[r][v]) - shift[v];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            int nc = 0;
#pragma unroll
            for (int r = 0; r < GM_R; ++r) nc += c[r] == g;
            if (nc == 0) continue;                         // wave-uniform
            const long long na = cnt[g], nt = na + nc;
            const double inv = 1.0 / (double)nc, w = (double)nc / (double)nt, f = (double)na * (double)nc / (double)nt;
#pragma unroll
            for (int v = 0; v < GM_V; ++v) {
                double s = 0.0, q = 0.0;
#pragma unroll
                for (int r = 0; r < GM_R; ++r)
                    if (c[r] == g) s += d[r][v];
                const double mc = s * inv;
#pragma unroll
                for (int r = 0; r < GM_R; ++r)
                    if (c[r] == g) {
                        const double e = d[r][v] - mc;
                        q = fma(e, e, q);
                    }
                const double dl = mc - mean[g][v];
                mean[g][v] = fma(dl, w, mean[g][v]);       // n = 0: w is 1 and the mean becomes mc exactly
                m2[g][v] += q + dl * dl * f;               // n = 0: f is 0; one row: q is 0 exactly
            }
            cnt[g] = nt;
        }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const long long o = ((long long)slice * NG + g) * n_sel;
#pragma unroll
        for (int v = 0; v < GM_V; ++v)
            if (j0 + v < n_sel) {
                pmean[o + j0 + v] = shift[v] + mean[g][v];
                pm2[o + j0 + v] = m2[g][v];
            }
        if (blockIdx.x == 0 && lane == 0) pcount[(long long)slice * NG + g] = cnt[g];
    }
}

// One thread per (group, selected column): Chan's update over the slices in slice order.  ng_stride: the NG the partials were
// written with.  An empty group gives count 0 and NaN.
__global__ void __launch_bounds__(256) group_moments_join_kernel(const long long *__restrict__ pcount, const double *__restrict__ pmean,
                                                                 const double *__restrict__ pm2, int n_slices, int ng_stride,
                                                                 int n_groups, int n_sel, long long *__restrict__ count,
                                                                 double *__restrict__ mean, double *__restrict__ m2) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_groups * n_sel) return;
    const int g = (int)(t / n_sel), j = (int)(t % n_sel);
    long long na = 0;
    double mu = 0.0, q = 0.0;
    for (int s = 0; s < n_slices; ++s) {
        const long long ns = pcount[(long long)s * ng_stride + g];
        if (ns == 0) continue;
        const long long o = ((long long)s * ng_stride + g) * n_sel + j, nt = na + ns;
        const double dl = pmean[o] - mu;
        mu = fma(dl, (double)ns / (double)nt, mu);
        q += pm2[o] + dl * dl * ((double)na * (double)ns / (double)nt);
        na = nt;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    mean[t] = na ? mu : nan;
    m2[t] = na ? q : nan;
    if (j == 0) count[g] = na;
}

}  // namespace pilot
