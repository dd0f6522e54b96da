// Cell-level W2 (C ABI: the cell cohort and its grid; include/pilot_ot.h).  Kernels: cellw2_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "abi_common.hpp"
#include "cellw2_kernels.hpp"

// cell-level W2 (extension)
struct pilot_ot_cell_cohort {
    int N = 0, D = 0, KB = 1, device = 0, n_cu = 256;
    long long C = 0, max_n = 0;
    float *dX = nullptr;           // the cells as given (resident: the operand pieces are rebuilt when scale * reg changes)
    float xb_scale = 0.f;          // operand scale the pieces were built with (0: not built)
    int xb_half = -1;              // ... and their format: 1 two fp16 pieces, 0 three bf16 pieces
    int xb_one_slot = -1;          // ... and whether the last k-slot of every cell holds 1 (cell_setup_kernel)
    float max_abs = 0.f;           // largest |coordinate| of the centred cohort (decides whether fp16 pieces are safe)
    double max_norm = 0.0;         // largest |x - mean| of the cohort, in fp64 (bounds the accuracy envelope: CELL_MAX_SCALED_NORM)
    uint4 *dXb = nullptr;          // bf16 operand pieces of every cell (resident)
    float *dnrm = nullptr;
    long long *doffs = nullptr;
    // per-call outputs / queue, grown on demand
    double *dW = nullptr, *dErr = nullptr;
    int *dIt = nullptr, *dQ = nullptr;
    size_t n_out = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

PILOT_API int pilot_ot_cell_cohort_destroy(pilot_ot_cell_cohort *c) {
    if (!c) return PILOT_OT_OK;
    for (void *p : {(void *)c->dX, (void *)c->dXb, (void *)c->dnrm, (void *)c->doffs, (void *)c->dW, (void *)c->dErr, (void *)c->dIt, (void *)c->dQ})
        if (p) (void)hipFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    delete c;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_cell_cohort_create(const float *X, const long long *offsets, int N, int D, pilot_ot_cell_cohort **cohort) {
    if (!X || !offsets || !cohort) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (N <= 0 || D <= 0) return fail(PILOT_OT_EINVAL, "N=%d D=%d must be positive", N, D);
    if (D > 64) return fail(PILOT_OT_ENOTSUP, "D=%d > 64 embedding dimensions", D);
    long long max_n = 0;
    for (int i = 0; i < N; ++i) {
        const long long n = offsets[i + 1] - offsets[i];
        if (n <= 0) return fail(PILOT_OT_EINVAL, "patient %d has %lld cells", i, n);
        if (n > max_n) max_n = n;
    }
    const size_t lds = sizeof(float) * (3 * (size_t)max_n + 48);
    if (lds > pilot::LDS_BYTES) return fail(PILOT_OT_ENOTSUP, "a patient with %lld cells needs %zu B of LDS (> %zu)", max_n, lds, pilot::LDS_BYTES);
    pilot_ot_cell_cohort *c = new (std::nothrow) pilot_ot_cell_cohort();
    if (!c) return fail(PILOT_OT_EINVAL, "out of host memory");
    c->N = N; c->D = D; c->KB = D <= 32 ? 1 : 2; c->C = offsets[N]; c->max_n = max_n;
    c->n_cu = pilot::cu_count();
    hipError_t e = hipGetDevice(&c->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->dX), sizeof(float) * (size_t)c->C * D);
    // (+ a zeroed pad: the pipelined column sweep of the fp16-piece kernel reads up to 31 cells past a patient's last one,
    // pilot::CELL_PAD_BYTES in cellw2_kernels.hpp)
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->dXb), (size_t)c->C * c->KB * 3 * 64 + pilot::CELL_PAD_BYTES);
    if (e == hipSuccess) e = hipMemset(c->dXb, 0, (size_t)c->C * c->KB * 3 * 64 + pilot::CELL_PAD_BYTES);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->dnrm), sizeof(float) * (size_t)c->C);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->doffs), sizeof(long long) * (size_t)(N + 1));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->dQ), sizeof(int));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) {
        // |x - y|^2 does not change when every cell is shifted by the same vector, but the f32 cancellation in
        // |x|^2 + |y|^2 - 2 <x, y> does: the cohort is stored centred on its mean (computed in fp64)
        std::vector<double> mean((size_t)D, 0.0);
        for (long long i = 0; i < c->C; ++i)
            for (int d = 0; d < D; ++d) mean[(size_t)d] += (double)X[(size_t)i * D + d];
        for (int d = 0; d < D; ++d) mean[(size_t)d] /= (double)c->C;
        std::vector<float> Xc((size_t)c->C * D);
        float mx = 0.f;
        double mn2 = 0.0;
        for (long long i = 0; i < c->C; ++i) {
            double n2 = 0.0;
            for (int d = 0; d < D; ++d) {
                const double vd = (double)X[(size_t)i * D + d] - mean[(size_t)d];
                const float v = (float)vd;
                Xc[(size_t)i * D + d] = v;
                mx = fabsf(v) > mx ? fabsf(v) : mx;
                n2 += vd * vd;
            }
            mn2 = n2 > mn2 ? n2 : mn2;
        }
        c->max_abs = mx;
        c->max_norm = sqrt(mn2);
        e = hipMemcpy(c->dX, Xc.data(), sizeof(float) * (size_t)c->C * D, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemcpy(c->doffs, offsets, sizeof(long long) * (size_t)(N + 1), hipMemcpyHostToDevice);
    if (e != hipSuccess) { pilot_ot_cell_cohort_destroy(c); return fail(PILOT_OT_EHIP, "cell cohort setup failed: %s", hipGetErrorString(e)); }
    *cohort = c;
    return PILOT_OT_OK;
}

namespace {
// enqueue one pass over the selected rows on the cohort's stream (asynchronous)
int cell_w2_enqueue(pilot_ot_cell_cohort *c, double scale, double reg, int num_iter_max, double stop_thr, int check_period,
                    double f32_floor_ulps, int row_begin, int row_end, int row_step, size_t *n_out_p) {
    if (!c) return fail(PILOT_OT_EINVAL, "cohort is NULL");
    if (!(scale > 0.0) || !(reg > 0.0)) return fail(PILOT_OT_EINVAL, "scale=%g reg=%g must be positive", scale, reg);
    if (num_iter_max < 1 || check_period < 1) return fail(PILOT_OT_EINVAL, "num_iter_max / check_period must be >= 1");
    if (row_step < 1 || row_begin < 0 || row_end > c->N || row_begin > row_end)
        return fail(PILOT_OT_EINVAL, "bad row range [%d, %d) step %d for N=%d", row_begin, row_end, row_step, c->N);
    {
        // accuracy envelope: the exponent of a pair is an f32 sum of terms of size s_i s_j (s: a cell's scaled norm), so one
        // far-out cell costs accuracy that the plan does not average away (pilot::CELL_MAX_SCALED_NORM)
        const double s_max = c->max_norm * sqrt(2.0 * 1.4426950408889634 / (scale * reg));
        if (s_max > pilot::CELL_MAX_SCALED_NORM)
            return fail(PILOT_OT_ENOTSUP, "a cell lies too far out for the f32 kernel: max_i |x_i - mean| * sqrt(2 log2(e) / (scale * reg)) "
                        "= %.4g > %g (drop far-out cells, or raise scale or reg)", s_max, pilot::CELL_MAX_SCALED_NORM);
    }
    const int n_rows = (row_end - row_begin + row_step - 1) / row_step;
    const size_t n_out = (size_t)n_rows * c->N;
    *n_out_p = n_out;
    if (n_out == 0) return PILOT_OT_OK;
    if (!(f32_floor_ulps > 0.0)) f32_floor_ulps = 8.0;
    if (n_out > c->n_out) {
        for (void *p : {(void *)c->dW, (void *)c->dErr, (void *)c->dIt}) if (p) (void)hipFree(p);
        c->dW = c->dErr = nullptr; c->dIt = nullptr; c->n_out = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->dW), sizeof(double) * n_out);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->dErr), sizeof(double) * n_out);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->dIt), sizeof(int) * n_out);
        if (e != hipSuccess) return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e));
        c->n_out = n_out;
    }
    HIP_TRY(hipMemsetAsync(c->dQ, 0, sizeof(int), c->stream));
    pilot::CellParams p;
    p.Xb = c->dXb; p.C = c->C; p.nrm = c->dnrm; p.offs = c->doffs; p.N = c->N;
    p.n_rows = n_rows; p.row_begin = row_begin; p.row_step = row_step;
    int half = 0;
    const double alpha = 1.0 / (scale * reg);
    p.alpha = (float)alpha;
    p.two_alpha2 = (float)(2.0 * alpha * 1.4426950408889634);
    {
        // operand pieces of sqrt(2 alpha log2 e) * x: a dot product of two operands is the exponent term itself
        const float op_scale = sqrtf(p.two_alpha2);
        p.two_alpha2 = op_scale * op_scale;
        p.dot_unscale = 1.f / p.two_alpha2;
        // two fp16 pieces (half the matrix work) while the scaled coordinates stay far inside fp16's range and above the
        // level where its subnormal spacing (2^-24) would cost accuracy; three bf16 pieces otherwise (PILOT_OT_CELL_BF16=1: always;
        // below the CELL_MAX_SCALED_NORM refusal above, only the switch selects them)
        const char *force = pilot::test_switch("PILOT_OT_CELL_BF16");
        half = c->max_abs * op_scale < 3.0e4f && !(force && *force && *force != '0') ? 1 : 0;
        const int one_slot = half && c->D <= 32 * c->KB - 2 && !pilot::test_switch("PILOT_OT_CELL_NO_AUG") ? 1 : 0;
        if (c->xb_scale != op_scale || c->xb_half != half || c->xb_one_slot != one_slot) {
            if (c->xb_half != half) HIP_TRY(hipMemsetAsync(c->dXb, 0, (size_t)c->C * c->KB * 3 * 64 + pilot::CELL_PAD_BYTES, c->stream));   // (the piece count changes the planes)
            hipLaunchKernelGGL(pilot::cell_setup_kernel, dim3(pilot::grid_for(c->C * c->KB * 32, 256, c->n_cu)), dim3(256), 0, c->stream, c->dX,
                               (long)c->C, c->D, c->KB, op_scale, half, one_slot, reinterpret_cast<unsigned short *>(c->dXb), c->dnrm);
            HIP_TRY(hipGetLastError());
            c->xb_scale = op_scale;
            c->xb_half = half;
            c->xb_one_slot = one_slot;
        }
    }
    p.inv_scale = (float)(1.0 / scale);
    p.max_iter = num_iter_max; p.period = check_period;
    p.stop_thr = (float)stop_thr; p.floor_ulps = (float)f32_floor_ulps;
    p.max_n = (int)c->max_n;
    p.w2 = c->dW; p.iters = c->dIt; p.err = c->dErr; p.queue = c->dQ;
    const size_t lds = sizeof(float) * (3 * (size_t)c->max_n + 48);
    long wgs = (long)n_out;
    long per_cu = (long)(pilot::LDS_BYTES / lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
    if (wgs > c->n_cu * per_cu) wgs = c->n_cu * per_cu;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    hipError_t le = hipSuccess;
    const bool aug = c->D <= 32 * c->KB - 2 && !pilot::test_switch("PILOT_OT_CELL_NO_AUG");      // two spare k-slots carry h_col - m_row
    auto launch = [&](auto kern) {
        le = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (le == hipSuccess) hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(pilot::CELL_WG), lds, c->stream, p);
    };
    if (half) {
        if (c->KB == 1) { if (aug) launch(pilot::cell_w2_kernel<1, true, true>); else launch(pilot::cell_w2_kernel<1, false, true>); }
        else            { if (aug) launch(pilot::cell_w2_kernel<2, true, true>); else launch(pilot::cell_w2_kernel<2, false, true>); }
    } else {
        if (c->KB == 1) { if (aug) launch(pilot::cell_w2_kernel<1, true>); else launch(pilot::cell_w2_kernel<1, false>); }
        else            { if (aug) launch(pilot::cell_w2_kernel<2, true>); else launch(pilot::cell_w2_kernel<2, false>); }
    }
    HIP_TRY(le);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    return PILOT_OT_OK;
}
int cell_w2_collect(pilot_ot_cell_cohort *c, size_t n_out, double *w2, int *iters, double *err, float *kernel_ms) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_out == 0) return PILOT_OT_OK;
    if (w2) HIP_TRY(hipMemcpy(w2, c->dW, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    if (iters) HIP_TRY(hipMemcpy(iters, c->dIt, sizeof(int) * n_out, hipMemcpyDeviceToHost));
    if (err) HIP_TRY(hipMemcpy(err, c->dErr, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, c->ev0, c->ev1));
    return PILOT_OT_OK;
}
}  // namespace

PILOT_API int pilot_ot_cell_w2_grid_cohort(pilot_ot_cell_cohort *c, double scale, double reg, int num_iter_max, double stop_thr,
                                           int check_period, double f32_floor_ulps, int row_begin, int row_end, int row_step,
                                           double *w2, int *iters, double *err, float *kernel_ms) {
    if (!c || !w2) return fail(PILOT_OT_EINVAL, "NULL pointer");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != c->device) HIP_TRY(hipSetDevice(c->device));
    size_t n_out = 0;
    int rc = cell_w2_enqueue(c, scale, reg, num_iter_max, stop_thr, check_period, f32_floor_ulps, row_begin, row_end, row_step, &n_out);
    if (rc == PILOT_OT_OK) rc = cell_w2_collect(c, n_out, w2, iters, err, kernel_ms);
    if (dev != c->device) (void)hipSetDevice(dev);
    return rc;
}

PILOT_API int pilot_ot_cell_cohort_pieces(pilot_ot_cell_cohort *c, int *pieces) {
    if (!c || !pieces) return fail(PILOT_OT_EINVAL, "NULL pointer");
    *pieces = c->xb_half < 0 ? 0 : (c->xb_half ? 2 : 3);      // operand pieces of the last call: 2 fp16, 3 bf16, 0 none yet
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_cell_w2_grid(const float *X, const long long *offsets, int N, int D, double scale, double reg,
                                    int num_iter_max, double stop_thr, int check_period, double f32_floor_ulps,
                                    int row_begin, int row_end, int row_step, double *w2, int *iters, double *err) {
    if (!X || !offsets || !w2) return fail(PILOT_OT_EINVAL, "NULL pointer");
    pilot_ot_cell_cohort *c = nullptr;
    int rc = pilot_ot_cell_cohort_create(X, offsets, N, D, &c);
    if (rc != PILOT_OT_OK) return rc;
    rc = pilot_ot_cell_w2_grid_cohort(c, scale, reg, num_iter_max, stop_thr, check_period, f32_floor_ulps, row_begin, row_end,
                                      row_step, w2, iters, err, nullptr);
    pilot_ot_cell_cohort_destroy(c);
    return rc;
}

// internal face of the cohort for the multi-device form (pilot_ot_multi.hip: row shards + device-side all-gather)
namespace pilot {
int cell_enqueue_rows(pilot_ot_cell_cohort *c, double scale, double reg, int num_iter_max, double stop_thr, int check_period,
                      double f32_floor_ulps, int row_begin, int row_end, int row_step, size_t *n_out) {
    return cell_w2_enqueue(c, scale, reg, num_iter_max, stop_thr, check_period, f32_floor_ulps, row_begin, row_end, row_step, n_out);
}
int cell_collect(pilot_ot_cell_cohort *c, size_t n_out, double *w2, int *iters, double *err, float *kernel_ms) {
    return cell_w2_collect(c, n_out, w2, iters, err, kernel_ms);
}
void cell_buffers(pilot_ot_cell_cohort *c, double **d_w2, hipStream_t *stream) { *d_w2 = c->dW; *stream = c->stream; }
}  // namespace pilot
