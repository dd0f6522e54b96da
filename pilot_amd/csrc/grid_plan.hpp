// The pair grid's host side, shared by pilot_ot_sinkhorn.hip and pilot_ot_emd.hip (and pilot_ot.hip, which owns the per-thread
// staging): the plan a device-resident call runs on, and the staging the host-buffer entry points keep per calling thread.
#pragma once
#include <hip/hip_runtime.h>

#include "abi_common.hpp"
#include "sinkhorn_layout.hpp"

constexpr int TIMING_RING = 64;

struct pilot_ot_plan {
    int N, K, device;
    double max_cost;   // max(M) of the cost the caller keeps on the device (pilot_ot_plan_set_max_cost; 1 = Trajectory.py:101's
                       // normalised cost): every range decision of a device-resident call is taken on max_cost / reg
    void *img;         // 3 operand images, sized for f64 at this K
    void *p_slot;      // N x KP proportions in accumulator-slot order (f32 or f64; sized for f64)
    int *track_list;   // N x N
    int *ctrl;         // TWO control blocks of CTRL_BLOCK_INTS ints each (slots named next to CTRL_INTS in sinkhorn_layout.hpp), zeroed at creation.
                       // An ordinary grid call works on block ctrl_par and its prep kernel zeroes the other one for the call after it;
                       // the calls that keep a memset of their own (the wide kernel, a captured graph) work on block 0
    int ctrl_par;      // block of the next ordinary grid call; flips when that call's prep launch has been issued
    int *order_list;   // N x N: longest-first work order of the fast launch
    unsigned char *order_bucket;  // N x N
    int *order_tiles;  // ORDER_NB bucket counts per order tile of the prep kernel (order_tile_count(N, N) tiles), read by the scatter
    int *flags_ws;     // N x N per-pair flags when the caller passes none
    int *emd_counter;  // 1: dynamic pair queue of the exact-EMD kernel
    double *f_slab;    // exact-EMD flow values: one K*K block per resident wave (per 16-lane group of a wave for K <= 16); allocated by the
    size_t f_slab_bytes;  // first exact-mode call that needs it -- a Sinkhorn-only plan never pays for it (164 MB at K = 50)
    double *emdg_slab; // K > 256: flow + label slab per resident workgroup of emd_generic_kernel, then K row minima (lazy)
    int emdg_wgs;
    double *kws;       // generic Sinkhorn kernel: K' and its transpose per workgroup (allocated on first use)
    int generic_wgs;
    float *wide_rec;   // 128 < K <= 256: one record per pair of the grid for sinkhorn_wide_kernel (allocated on first use)
    size_t wide_rec_n; //   pairs it holds
    int *nan_list;     // 2 x N x N: pairs that ended in NaN, then pairs the f32 passes hand to the f64 pass
    int n_cu;
    // event ring for per-launch kernel timing (bench.py roofline)
    int timing;                       // 0 off
    long n_timed;                     // calls recorded so far
    long n_calls;                     // calls seen while timing is on (every `timing`-th one is recorded)
    hipEvent_t ev[TIMING_RING][3];    // [slot]{main begin, main end = track begin, track end}
    // hipGraph replay of a repeated Sinkhorn call (pilot_ot_plan_enable_graph): the launch sequence of one call captured
    // on `gstream` and replayed on the caller's stream while the arguments stay the same
    int graph_mode;                   // 0 off
    int gkey_seen;                    // the key below was used by an ordinary (uncaptured) call: buffers are grown
    struct GraphKey {
        const void *P, *M, *emd, *iters, *err, *flags;
        double reg, stop_thr, tau, floor_ulps, max_cost;
        int num_iter_max, check_period, cfg, mixed, sym, row_begin, n_rows, row_step;
        pilot::SinkhornSwitches sw;
        bool operator==(const GraphKey &o) const {
            return P == o.P && M == o.M && emd == o.emd && iters == o.iters && err == o.err && flags == o.flags && reg == o.reg &&
                   stop_thr == o.stop_thr && tau == o.tau && floor_ulps == o.floor_ulps && max_cost == o.max_cost && num_iter_max == o.num_iter_max &&
                   check_period == o.check_period && cfg == o.cfg && mixed == o.mixed && sym == o.sym && row_begin == o.row_begin &&
                   n_rows == o.n_rows && row_step == o.row_step && sw == o.sw;
        }
    } gkey;
    hipStream_t gstream;
    hipGraphExec_t gexec;
};

namespace pilot {

// Host-buffer entry points keep one plan + staging buffers per calling thread and reuse them while the shape stays the same (a
// PILOT session calls with one (N, K)); pilot_ot_shutdown() releases them.
struct HostCtx {
    pilot_ot_plan *plan = nullptr;
    int N = 0, K = 0, device = -1;
    size_t n_out = 0;
    double *dP = nullptr, *dM = nullptr, *dE = nullptr, *dErr = nullptr;
    int *dIt = nullptr, *dFl = nullptr;
    // pinned staging of the results: a D2H copy straight into the caller's pageable arrays makes the driver pin and
    // unpin them on every call (measured: 2 ms -> 25 ms per c3 matrix whenever numpy hands out fresh pages)
    unsigned char *pin = nullptr;
    size_t pin_bytes = 0;
    // events behind the pieces of a large fetch (host_fetch): the copy out of the pinned block starts when the first piece lands
    static constexpr int FETCH_EVENTS = 32;
    hipEvent_t fev[FETCH_EVENTS];
    int n_fev = 0;
    void release() {
        for (int i = 0; i < n_fev; ++i) (void)hipEventDestroy(fev[i]);
        n_fev = 0;
        if (pin) (void)hipHostFree(pin);
        pin = nullptr; pin_bytes = 0;
        if (dP) (void)hipFree(dP);
        if (dM) (void)hipFree(dM);
        if (dE) (void)hipFree(dE);
        if (dErr) (void)hipFree(dErr);
        if (dIt) (void)hipFree(dIt);
        if (dFl) (void)hipFree(dFl);
        dP = dM = dE = dErr = nullptr; dIt = dFl = nullptr;
        if (plan) pilot_ot_plan_destroy(plan);
        plan = nullptr; N = K = 0; n_out = 0; device = -1;
    }
    ~HostCtx() {}   // device memory is released by pilot_ot_shutdown() or at process exit
};
HostCtx &thread_host();
// the calling thread's plan and staging, (re)made for this shape and at least n_out results
int host_ctx_prepare(int N, int K, size_t n_out);
// device results -> caller's arrays through the pinned staging block (entries with dst == nullptr are skipped)
struct Fetch { void *dst; const void *src; size_t bytes; };
int host_fetch(const Fetch *f, int n);

// bytes of pilot_ot_plan::emd_counter, the pair queue of the exact-OT kernels (pilot_ot_emd.hip)
size_t emd_counter_bytes();

}  // namespace pilot
