// Shared by the translation units that implement the C ABI: error reporting, test switches, the per-thread pool of device
// temporaries and the device limits every launch decision reads.  Host-side only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pilot_ot.h"
#include "sinkhorn_layout.hpp"     // LDS_BYTES

#define PILOT_API extern "C" __attribute__((visibility("default")))

namespace pilot {

// record the calling thread's error message (pilot_ot_last_error) and return `code`
int abi_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// value of a test switch (pilot_ot_test_switch), or nullptr: how the GPU tests and the A/B tools force a kernel variant.  The
// library reads NO environment variable that changes what it computes.
const char *test_switch(const char *name);
// release every cached multi-GPU context of the host-buffer entry points (called by pilot_ot_shutdown)
void abi_multi_release();

// The calling thread's pool of device temporaries: one buffer per slot, grown on demand, released by pilot_ot_shutdown.  Every
// buffer of every translation unit has a slot of its own here, so two buffers that are live together (diffmap chains into the
// consumer entry points) never share one.
// The list of slots: the enum below and the name table (pilot_ot_ws_slot_name) both expand these lines, so they cannot disagree.
#define PILOT_WS_SLOT_LIST(X) \
    X(WS_PREPASS_X) X(WS_PREPASS) \
    X(WS_COST_X) X(WS_COST_C) X(WS_COST_AUX) \
    X(WS_CONS_E) X(WS_CONS_D) X(WS_CONS_MAX) X(WS_CONS_LABELS) X(WS_CONS_SIZES) X(WS_CONS_SCORES) X(WS_CONS_K) \
    X(WS_PLAN_P) X(WS_PLAN_M) X(WS_PLAN_PI) X(WS_PLAN_PJ) X(WS_PLAN_VAL) X(WS_PLAN_IT) X(WS_PLAN_FL) X(WS_PLAN_Q) \
    X(WS_PLAN_PLANS) X(WS_PLAN_SLAB) X(WS_PLAN_ROWMIN) X(WS_PLAN_KWS) X(WS_PLAN_ACC) X(WS_PLAN_GOFF) X(WS_PLAN_GIDX) \
    X(WS_DM_S) X(WS_DM_V) X(WS_DM_VEC) X(WS_DM_Z) X(WS_DM_PSI) X(WS_DM_E) X(WS_DM_D) X(WS_DM_K) X(WS_DM_MAX) X(WS_DM_OUT) \
    X(WS_TF_U) X(WS_TF_Y) X(WS_TF_OUT) X(WS_TF_COLS) \
    X(WS_BOOT_U) X(WS_BOOT_OUT) X(WS_BOOT_IDX) X(WS_BOOT_Y) \
    X(WS_CV_Y) X(WS_CV_IN) X(WS_CV_AUX) X(WS_CV_OUT) X(WS_CV_BMAX) X(WS_CV_CHAIN) X(WS_CV_Z) \
    X(WS_GM_Y) X(WS_GM_AUX) X(WS_GM_PART) X(WS_GM_COUNT) X(WS_GM_OUT) \
    X(WS_CSR_COUNTS) X(WS_CSR_TOTAL) X(WS_CSR_CODES) X(WS_CSR_COLS) X(WS_CSR_OUT) \
    X(WS_GS_Y) X(WS_GS_AUX) X(WS_GS_PART) X(WS_GS_OUT) \
    X(WS_PCA_V) X(WS_PCA_VEC) X(WS_PCA_Z) X(WS_PCA_PCS) X(WS_PCA_SCORES) X(WS_PCA_STATS) X(WS_PCA_COLS) X(WS_PCA_POS) \
    X(WS_PCA_SIDX) X(WS_PCA_SVAL) X(WS_PCA_CSVAL) X(WS_PCA_Y) X(WS_PCA_S) X(WS_PCA_PARTW) \
    X(WS_KNN_X) X(WS_KNN_UNIT) X(WS_KNN_FLAGS) X(WS_KNN_BEST_D) X(WS_KNN_BEST_I) X(WS_KNN_OUT_D) X(WS_KNN_OUT_I) X(WS_KNN_SM_IN) X(WS_KNN_SM_OUT) \
    X(WS_LV_VAL0) X(WS_LV_VAL1) X(WS_LV_DEG0) X(WS_LV_DEG1) X(WS_LV_IDX0) X(WS_LV_IDX1) X(WS_LV_TOT) X(WS_LV_SUMS) X(WS_LV_INT) X(WS_LV_FLAG) X(WS_LV_ECOMM) \
    X(WS_LV_NKEYS) X(WS_LV_EKEYS) X(WS_LV_CNT) X(WS_LD_INT) X(WS_LD_DBL) \
    X(WS_SIL_X) X(WS_SIL_UNIT) X(WS_SIL_FLAGS) X(WS_SIL_SORTED) X(WS_SIL_ORDER) X(WS_SIL_OFFSETS) X(WS_SIL_OUT) \
    X(WS_PT_X) X(WS_PT_FLAGS) X(WS_PT_Y) X(WS_PT_YT) X(WS_PT_S) X(WS_PT_CENTRE) X(WS_PT_STATE) X(WS_PT_ITERS) X(WS_PT_ENERGY) X(WS_PT_COUNTS) X(WS_PT_SUMS) \
    X(WS_PT_PCOUNTS) X(WS_PT_PSUMS) X(WS_PT_PMSE) X(WS_PT_PART) X(WS_PT_OUT) \
    X(WS_RS_Y) X(WS_RS_INT) X(WS_RS_LL) X(WS_RS_REC) X(WS_RS_OUT) \
    X(WS_NB_Y) X(WS_NB_INT) X(WS_NB_SF) X(WS_NB_BAD) X(WS_NB_PRIOR) X(WS_NB_OUT) X(WS_NB_FIT_INT)
// (by prefix: PREPASS pilot_ot_prepass.hip, COST _cost, CONS _consumers, PLAN _plans, DM _diffmap, TF _trajfit, BOOT _bootfit, CV _curves,
//  GM _moments, CSR _csr, GS _group_sums, PCA _pca, KNN _knn, LV _louvain and LD the refinement of pilot_ot_leiden, SIL _silhouette_points,
//  PT _principal_tree, RS _rank_sums, NB _nb_glm)
enum WsSlot {
#define PILOT_WS_SLOT_ENUM(name) name,
    PILOT_WS_SLOT_LIST(PILOT_WS_SLOT_ENUM)
#undef PILOT_WS_SLOT_ENUM
    WS_SLOTS
};
// CONTRACT: a hand-out is an UNDEFINED buffer of `bytes` bytes.  Whatever an earlier hand-out of the slot held is gone (the pool may
// have regrown it, and under the test switch PILOT_OT_WS_GUARD every hand-out is filled with 0xFF and followed by a canary), so a
// caller writes every byte a kernel or a copy will read, addresses nothing past `bytes`, and keeps the pointer instead of asking
// for the same slot again while it still needs the contents.  pilot_ot_ws_guard_report tells what the guard saw.
hipError_t ws_buffer(WsSlot slot, size_t bytes, void **out);
// n elements of T (at least one) from `slot`
template <typename T> hipError_t ws(WsSlot slot, size_t n, T **out) {
    void *p = nullptr;
    const hipError_t e = ws_buffer(slot, sizeof(T) * (n ? n : 1), &p);
    *out = static_cast<T *>(p);
    return e;
}

// ---- dense matrix arguments: what every entry point that takes a row-major matrix (dtype code, columns, leading dimension, an
// optional column selection; on the host or in HBM) checks and stages.  The checks make no HIP call.
inline size_t elem_size(int dtype) { return dtype == 0 ? sizeof(float) : sizeof(double); }
int check_dtype(int dtype);
int check_ld(long long ld, int n_cols);
// a selection of n_sel columns out of n_cols: every cols[j] in range; without cols the selection is all of them
int check_cols(const int *cols, int n_sel, int n_cols);
// `rows` x `n_cols` elements of `es` bytes at Y, leading dimension ld, as a device pointer: Y and ld themselves when Y is in HBM,
// else a packed copy (leading dimension n_cols) in `slot`.  Chunked callers pass each chunk's first element and row count.
int stage_dense(const void *Y, int is_device, size_t es, long long rows, long long n_cols, long long ld, WsSlot slot, const void **ptr,
                long long *ld_out);
// the same for a whole packed float64 matrix of `count` elements
int stage_f64(const double *src, int is_device, size_t count, WsSlot slot, const double **out);

// device time of the calling thread's last pre-pass (pilot_ot_prepass_device_ms): two events on the launch stream
struct PrepassClock {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool valid = false;
    void release() { for (auto &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; } valid = false; }
    void start() {
        valid = false;
        if (!ev[0] && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) { release(); return; }
        (void)hipEventRecord(ev[0], nullptr);
    }
    void stop() { if (ev[1]) valid = hipEventRecord(ev[1], nullptr) == hipSuccess; }
};
PrepassClock &thread_clock();

// compute units of the current device (256 if the runtime cannot tell)
int cu_count();
// blocks of `block` threads for n items, at most 8 per CU
inline int grid_for(long n, int block, int n_cu) {
    long g = (n + block - 1) / block;
    const long cap = (long)n_cu * 8;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

constexpr int MAX_K = 128;          // the MFMA pair-grid kernels (8 row-tiles of 16 cell types)
constexpr int GENERIC_MAX_K = 2048;  // the reference-semantics fallback kernel (vectors in LDS)
constexpr int EMD_MAX_K = 256;       // exact-OT kernel: 4 rows / columns per lane
constexpr int WIDE_MAX_K = 256;      // sinkhorn_wide_kernel: 128 < K <= 256, eight waves per 16-pair tile

// the kNN kernel sorts a row in LDS, padded to the next power of two: 16384 doubles = 128 KiB is the largest that fits.  Every
// entry point that reaches the kernel asks this first, the host forms before they stage their N x N buffers.
inline int knn_rows_supported(int N) {
    return N <= PILOT_OT_KNN_MAX_N ? PILOT_OT_OK
                                   : abi_fail(PILOT_OT_ENOTSUP, "N=%d rows do not fit the LDS sort (at most %d)", N, PILOT_OT_KNN_MAX_N);
}

// cell-level cohort, internal face used by the multi-device form (pilot_ot_multi.hip)
int cell_enqueue_rows(pilot_ot_cell_cohort *c, double scale, double reg, int num_iter_max, double stop_thr, int check_period,
                      double f32_floor_ulps, int row_begin, int row_end, int row_step, size_t *n_out);
int cell_collect(pilot_ot_cell_cohort *c, size_t n_out, double *w2 /* nullable */, int *iters, double *err, float *kernel_ms);
void cell_buffers(pilot_ot_cell_cohort *c, double **d_w2, hipStream_t *stream);

}  // namespace pilot

#define fail(...) pilot::abi_fail(__VA_ARGS__)

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return pilot::abi_fail(PILOT_OT_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                   __FILE__, __LINE__);                                                    \
    } while (0)
