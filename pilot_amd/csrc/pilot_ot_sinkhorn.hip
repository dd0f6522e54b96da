// Entropic OT over the pair grid (C ABI: precision selection, plans, pilot_ot_sinkhorn_grid*, graph replay and kernel timing;
// include/pilot_ot.h).  Kernels: sinkhorn_kernels.hpp and its instantiations (sk_inst.hip, sk_wide.hip), generic_kernels.hpp.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "abi_common.hpp"
#include "grid_plan.hpp"
#include "sinkhorn_launch.hpp"
#include "generic_kernels.hpp"

namespace {
using pilot::LDS_BYTES, pilot::MAX_K, pilot::GENERIC_MAX_K, pilot::WIDE_MAX_K;

// does the bf16-split tracking kernel fit LDS at this K with a ring of four and the hand-over buffers its launch reserves?
// (the fp16-split configuration needs less for its fast pass and the same for its tracking pass)
bool split_fits_lds(int K, bool sym, int bands = 1) {
    const pilot::CfgShape c = pilot::shape_of(pilot::CFG_S32);
    return pilot::stream_layout(c, (K + 15) / 16, sym, true, 0, bands, 4).bytes + (size_t)pilot::handover_elems(c) * 4 <= LDS_BYTES;
}
}  // namespace

// ------------------------------------------------------------------------------------------------
// range of the fp16-split configuration (PILOT_OT_H_MAX_COST_OVER_REG: experiment switch of tools/f16x2_range_probe.py)
static double h_max_cost_over_reg() {
    const char *e = pilot::test_switch("PILOT_OT_H_MAX_COST_OVER_REG");
    return e && *e ? atof(e) : pilot::H_MAX_COST_OVER_REG;
}

PILOT_API int pilot_ot_auto_precision(double max_cost_over_reg) {
    // f32 keeps every Gibbs-kernel entry exp(-M/reg) a well-scaled normal number only while
    // max(M)/reg stays clear of the f32 exponent range (ln FLT_MIN = -87.3); beyond ~60 the
    // far-transport entries lose bits, so AUTO switches to the f64 kernel.
    // Inside that range the f32 values are iterated with bf16-split products (PILOT_OT_PREC_BF16X3: f32-level rounding on
    // the bf16 matrix pipe, measured 1.3x the f32-input MFMA path).
    // While max(M)/reg <= 16 (PILOT's default reg = 0.1 on the max-normalised cost gives 10) every entry of 2^15 exp(-M/reg)
    // is a fp16 pair good to <= 2^-15.9 relative (22 bits down to 11.8; see H_MAX_COST_OVER_REG) and the products run on 2-way fp16 splits (PILOT_OT_PREC_F16X2: half the MFMAs, a third of
    // the split instructions of BF16X3; same stopping checks, same 1e-7 class distance to the fp64 oracle).
    if (max_cost_over_reg <= h_max_cost_over_reg()) return PILOT_OT_PREC_F16X2;
    return max_cost_over_reg <= 60.0 ? PILOT_OT_PREC_BF16X3 : PILOT_OT_PREC_F64;
}

PILOT_API int pilot_ot_auto_precision_for(double max_cost_over_reg, int K, int cost_is_symmetric) {
    int prec = pilot_ot_auto_precision(max_cost_over_reg);
    if ((prec == PILOT_OT_PREC_BF16X3 || prec == PILOT_OT_PREC_F16X2) && !split_fits_lds(K, cost_is_symmetric != 0, 1)) prec = PILOT_OT_PREC_F32;
    return prec;
}

// The one place where a requested precision becomes the precision a call runs (host, multi-device and device entry points):
//  * exp(-max(M)/reg) outside the f64 range, or on request -> POT-literal kernel;
//  * AUTO -> F16X2 / BF16X3 by range (F32 where the split images do not fit LDS), AUTO_MIXED beyond the f32 range;
//  * an explicit f32-class precision beyond the f32 range (max(M)/reg > 60) would be off by up to 1e-4 on this path's
//    distributions: it runs AUTO_MIXED as well -- explicit precisions are honoured inside their valid range only;
//  * F16X2 outside its scaled domain (cost range, tau) -> BF16X3.
PILOT_API int pilot_ot_resolve_precision(int precision, double max_cost_over_reg, int K, int cost_is_symmetric, double tau) {
    if (precision == PILOT_OT_PREC_GENERIC || max_cost_over_reg > PILOT_OT_MAX_COST_OVER_REG) return PILOT_OT_PREC_GENERIC;
    const bool f32_class = precision == PILOT_OT_PREC_F32 || precision == PILOT_OT_PREC_BF16X3 || precision == PILOT_OT_PREC_F16X2;
    // (PILOT_OT_RAW_PRECISION=1, tests only: run an explicit f32-class precision outside its range as asked)
    const char *raw = pilot::test_switch("PILOT_OT_RAW_PRECISION");
    const bool promote = f32_class && max_cost_over_reg > 60.0 && !(raw && *raw && *raw != '0');
    if (precision == PILOT_OT_PREC_AUTO || promote) {
        precision = pilot_ot_auto_precision_for(max_cost_over_reg, K, cost_is_symmetric);
        if (precision == PILOT_OT_PREC_F64) precision = PILOT_OT_PREC_AUTO_MIXED;    // f32 first, f64 for the pairs that need it
    }
    if (precision == PILOT_OT_PREC_F16X2 &&
        (max_cost_over_reg > h_max_cost_over_reg() || tau > pilot::H_MAX_TAU || !split_fits_lds(K, cost_is_symmetric != 0, 1)))
        precision = split_fits_lds(K, cost_is_symmetric != 0, 1) ? PILOT_OT_PREC_BF16X3 : PILOT_OT_PREC_F32;
    return precision;
}

PILOT_API int pilot_ot_plan_create(int N, int K, pilot_ot_plan **plan) {
    if (!plan) return fail(PILOT_OT_EINVAL, "plan is NULL");
    if (N <= 0 || K <= 0) return fail(PILOT_OT_EINVAL, "N=%d K=%d must be positive", N, K);
    if (K > GENERIC_MAX_K) return fail(PILOT_OT_ENOTSUP, "K=%d > %d cell types", K, GENERIC_MAX_K);
    if ((long long)N * N > 0x7fffffffLL) return fail(PILOT_OT_ENOTSUP, "N=%d: N*N overflows the pair index", N);
    pilot_ot_plan *pl = new (std::nothrow) pilot_ot_plan();
    if (!pl) return fail(PILOT_OT_EINVAL, "out of host memory");
    pl->N = N; pl->K = K; pl->max_cost = 1.0;
    pl->img = nullptr; pl->p_slot = nullptr; pl->track_list = nullptr; pl->ctrl = nullptr;
    pl->emd_counter = nullptr; pl->f_slab = nullptr; pl->f_slab_bytes = 0; pl->emdg_slab = nullptr; pl->emdg_wgs = 0; pl->n_cu = 256; pl->kws = nullptr; pl->generic_wgs = 0; pl->nan_list = nullptr;
    pl->wide_rec = nullptr; pl->wide_rec_n = 0;
    pl->order_list = nullptr; pl->order_bucket = nullptr; pl->order_tiles = nullptr; pl->ctrl_par = 0;
    pl->flags_ws = nullptr;
    pl->timing = 0; pl->n_timed = 0; pl->n_calls = 0;
    pl->graph_mode = 0; pl->gkey_seen = 0; pl->gstream = nullptr; pl->gexec = nullptr;
    for (int i = 0; i < TIMING_RING; ++i) for (int j = 0; j < 3; ++j) pl->ev[i][j] = nullptr;
    hipError_t e = hipGetDevice(&pl->device);
    if (e == hipSuccess) pl->n_cu = pilot::cu_count();
    const int kp = ((K + 31) / 32) * 32;
    if (K <= MAX_K) {
        const int rt = (K + 15) / 16;
        size_t img_bytes = pilot::img_elems(pilot::CFG_F64, rt) * sizeof(double);
        const size_t b32 = pilot::img_elems(pilot::CFG_F32, rt) * sizeof(float), bs = pilot::img_elems(pilot::CFG_S32, rt) * sizeof(float);
        const size_t bh = pilot::img_elems(pilot::CFG_H32, rt) * sizeof(float);
        if (b32 > img_bytes) img_bytes = b32;
        if (bs > img_bytes) img_bytes = bs;
        if (bh > img_bytes) img_bytes = bh;
        if (e == hipSuccess) e = hipMalloc(&pl->img, img_bytes);
    } else if (K <= WIDE_MAX_K) {       // the 8-waves-per-tile kernel: the fp16-split operand block at 16 row-tiles
        if (e == hipSuccess) e = hipMalloc(&pl->img, pilot::img_elems(pilot::CFG_H32, 16) * sizeof(float));
    }
    {
        // proportions in slot order + one stop threshold per patient: sized for f64 at the padded K; the fp16-split configuration keeps
        // TWO f32 copies there (plain, and in its scaled domain) -- the same bytes up to K = 128, more with the 16 row-tiles of the
        // eight-waves-per-tile kernel
        size_t p_bytes = sizeof(double) * ((size_t)N * kp + N);
        if (K > MAX_K && K <= WIDE_MAX_K) { const size_t two = 2 * sizeof(float) * ((size_t)N * 256 + N); p_bytes = two > p_bytes ? two : p_bytes; }
        if (e == hipSuccess) e = hipMalloc(&pl->p_slot, p_bytes);
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&pl->track_list), sizeof(int) * (size_t)N * N);
    // (two control blocks, both zero from here on whenever a call finds them: see run_grid)
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&pl->ctrl), 2 * pilot::CTRL_BLOCK_INTS * sizeof(int));
    if (e == hipSuccess) e = hipMemset(pl->ctrl, 0, 2 * pilot::CTRL_BLOCK_INTS * sizeof(int));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // (the first call may come on a stream that does not wait for the null stream)
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&pl->order_tiles), sizeof(int) * pilot::ORDER_NB * (size_t)pilot::order_tile_count(N, N));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&pl->order_list), sizeof(int) * (size_t)N * N);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&pl->order_bucket), (size_t)N * N);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&pl->emd_counter), pilot::emd_counter_bytes());
    // per-pair work lists and flags of the full grid: a call has at most N x N pairs, so no grid call grows them (the POT-literal
    // kernel's scratch, 2 K^2 doubles per resident workgroup, and the wide kernel's records are allocated by the first call that
    // needs them)
    // (two lists of N^2: pairs that ended in NaN, and pairs the f32 passes hand to the f64 pass)
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&pl->nan_list), 2 * sizeof(int) * (size_t)N * N);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&pl->flags_ws), sizeof(int) * (size_t)N * N);
    if (e != hipSuccess) {
        pilot_ot_plan_destroy(pl);
        return fail(PILOT_OT_EHIP, "plan allocation failed: %s", hipGetErrorString(e));
    }
    *plan = pl;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_plan_set_max_cost(pilot_ot_plan *pl, double max_cost) {
    if (!pl) return fail(PILOT_OT_EINVAL, "plan is NULL");
    if (!(max_cost > 0.0) || !std::isfinite(max_cost)) return fail(PILOT_OT_EINVAL, "max_cost=%g must be positive and finite", max_cost);
    pl->max_cost = max_cost;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_plan_destroy(pilot_ot_plan *pl) {
    if (!pl) return PILOT_OT_OK;
    if (pl->img) (void)hipFree(pl->img);
    if (pl->p_slot) (void)hipFree(pl->p_slot);
    if (pl->track_list) (void)hipFree(pl->track_list);
    if (pl->ctrl) (void)hipFree(pl->ctrl);
    if (pl->order_list) (void)hipFree(pl->order_list);
    if (pl->order_bucket) (void)hipFree(pl->order_bucket);
    if (pl->order_tiles) (void)hipFree(pl->order_tiles);
    if (pl->flags_ws) (void)hipFree(pl->flags_ws);
    if (pl->emd_counter) (void)hipFree(pl->emd_counter);
    if (pl->f_slab) (void)hipFree(pl->f_slab);
    if (pl->emdg_slab) (void)hipFree(pl->emdg_slab);
    if (pl->kws) (void)hipFree(pl->kws);
    if (pl->nan_list) (void)hipFree(pl->nan_list);
    if (pl->wide_rec) (void)hipFree(pl->wide_rec);
    if (pl->gexec) (void)hipGraphExecDestroy(pl->gexec);
    if (pl->gstream) (void)hipStreamDestroy(pl->gstream);
    for (int i = 0; i < TIMING_RING; ++i) for (int j = 0; j < 3; ++j) if (pl->ev[i][j]) (void)hipEventDestroy(pl->ev[i][j]);
    delete pl;
    return PILOT_OT_OK;
}

namespace {

int check_grid_args(int N, int K, double reg, int num_iter_max, double stop_thr, double tau, int check_period,
                    int precision, int row_begin, int row_end, int row_step) {
    if (N <= 0 || K <= 0) return fail(PILOT_OT_EINVAL, "N=%d K=%d must be positive", N, K);
    if (!(reg > 0.0) || !std::isfinite(reg)) return fail(PILOT_OT_EINVAL, "reg=%g must be positive and finite", reg);
    if (num_iter_max < 1) return fail(PILOT_OT_EINVAL, "num_iter_max=%d must be >= 1", num_iter_max);
    if (check_period < 1) return fail(PILOT_OT_EINVAL, "check_period=%d must be >= 1", check_period);
    if (!(stop_thr >= 0.0) || !(stop_thr < 1.0)) return fail(PILOT_OT_EINVAL, "stop_thr=%g must be in [0, 1)", stop_thr);
    if (!(tau > 1.0)) return fail(PILOT_OT_EINVAL, "tau=%g must be > 1", tau);
    if (precision < PILOT_OT_PREC_AUTO || precision > PILOT_OT_PREC_F16X2)
        return fail(PILOT_OT_EINVAL, "unknown precision id %d", precision);
    if (row_step < 1 || row_begin < 0 || row_end > N || row_begin > row_end)
        return fail(PILOT_OT_EINVAL, "bad row range [%d, %d) step %d for N=%d", row_begin, row_end, row_step, N);
    if (K > GENERIC_MAX_K) return fail(PILOT_OT_ENOTSUP, "K=%d > %d cell types", K, GENERIC_MAX_K);
    return PILOT_OT_OK;
}

// The MFMA kernels iterate TOTAL scalings against the fixed Gibbs image exp(-M/reg) (POT's log-absorption is value-neutral
// and only its bookkeeping is tracked), so max(M)/reg must stay inside the exponent range of the widest type: beyond ~600
// an f64 Gibbs entry underflows / a total scaling overflows where POT's absorbed kernel would not.  Such calls, and K > 128,
// go to the reference-semantics kernel (generic_kernels.hpp), which rebuilds the absorbed kernel like POT.
constexpr double MAX_COST_OVER_REG = PILOT_OT_MAX_COST_OVER_REG;

// The two control blocks of a plan.  Both are zero when the plan is made.  An ordinary grid call (run_grid outside graph capture)
// works on block ctrl_par and has its prep kernel zero the other one, which nothing reads meanwhile; the parity flips once
// that prep launch is issued, so the next call finds its block zero without a memset.  A call that returns before that launch
// (argument error, empty row range, a shape handed to the POT-literal kernel) leaves the parity alone.
int *ctrl_block(const pilot_ot_plan *pl, int which) { return pl->ctrl + (size_t)which * pilot::CTRL_BLOCK_INTS; }
// The block that the next ordinary call does not read and zeroes itself: where a POT-literal call of its own keeps its queue head.
int *ctrl_spare(const pilot_ot_plan *pl) { return ctrl_block(pl, pl->ctrl_par ^ 1); }

// list / list_len (device, nullable): only the listed pairs (NaN hand-over of the fast kernels) with `queue`, their zeroed counter.
// Without a list: a call of its own, which zeroes and uses the slot CTRL_GENERIC_HEAD of the control block `own`.
int run_generic(pilot_ot_plan *pl, const pilot::SinkhornSwitches &sw, const double *d_P, const double *d_M, double reg, int num_iter_max, double stop_thr, double tau,
                int check_period, int row_begin, int n_rows, int row_step, double *d_emd, int *d_iters, double *d_err, int *d_flags,
                hipStream_t s, int *own, const int *list = nullptr, const int *list_len = nullptr, int *queue = nullptr) {
    const int N = pl->N, K = pl->K;
    const int n_pairs = n_rows * N;
    if (n_pairs == 0) return PILOT_OT_OK;
    // 8 vectors + nsplit rows of partial sums (as many as fit, a power of two <= the waves of a workgroup) + reduction scratch + queue slot
    int nsplit = pilot::GENERIC_WAVES;
    auto lds_for = [&](int ns) { return sizeof(double) * ((8 + (size_t)ns) * (size_t)K + pilot::GENERIC_WAVES) + 16; };
    while (nsplit > 1 && lds_for(nsplit) > LDS_BYTES) nsplit /= 2;
    const size_t lds = lds_for(nsplit);
    if (lds > LDS_BYTES) return fail(PILOT_OT_ENOTSUP, "K=%d does not fit the generic kernel's LDS vectors", K);
    if (!pl->kws) {
        // two workgroups per CU, fewer when K' and its transpose would take more than 8 GB in all
        int wgs = 3 * pl->n_cu;
        const size_t per = sizeof(double) * 2 * (size_t)K * K;
        while (wgs > 1 && per * wgs > ((size_t)8 << 30)) wgs /= 2;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pl->kws), per * wgs));
        pl->generic_wgs = wgs;
    }
    if (!queue) { queue = own + pilot::CTRL_GENERIC_HEAD; HIP_TRY(hipMemsetAsync(queue, 0, sizeof(int), s)); }
    pilot::GenericParams g;
    g.P = d_P; g.M = d_M; g.N = N; g.K = K; g.n_pairs = n_pairs; g.row_begin = row_begin; g.row_step = row_step;
    g.reg = reg; g.tau = tau; g.stop_thr = stop_thr; g.max_iter = num_iter_max; g.period = check_period;
    g.emd = d_emd; g.iters = d_iters; g.err = d_err; g.flags = d_flags; g.kws = pl->kws; g.queue = queue; g.nsplit = nsplit;
    g.list = list; g.list_len = list_len;
    int wgs = pl->generic_wgs < n_pairs ? pl->generic_wgs : n_pairs;
    if (list && wgs > 64) wgs = 64;          // a hand-over list is short (usually empty)
    if (sw.generic_wgs > 0 && sw.generic_wgs < wgs) wgs = sw.generic_wgs;      // experiment switch
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::sinkhorn_generic_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pilot::sinkhorn_generic_kernel, dim3(wgs), dim3(pilot::GENERIC_WG), lds, s, g);
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}

// The launch parameters run_grid and run_wide share: the whole call on the plan's buffers, in the longest-first order, drawn from
// the fast launch's queue head, with the control block `ctrl`.  Pairs that end in NaN ("Numerical errors" in POT) are collected and re-solved by the POT-literal
// kernel, which returns the last good iterate like POT does.
pilot::GridParams call_params(const pilot_ot_plan *pl, int *ctrl, int n_pairs, int row_begin, int row_step, int num_iter_max, int check_period,
                              double stop_thr, double tau, double floor_ulps, double *d_emd, int *d_iters, double *d_err, int *d_flags) {
    pilot::GridParams p;
    p.P = pl->p_slot; p.img = pl->img; p.N = pl->N; p.K = pl->K;
    p.n_pairs = n_pairs;
    p.list = pl->order_list; p.list_len = nullptr;
    p.solo_len = nullptr; p.solo_head = nullptr; p.solo_blocks = 0;
    p.row_begin = row_begin; p.row_step = row_step;
    p.max_iter = num_iter_max; p.period = check_period;
    p.stop_thr = stop_thr; p.tau = tau; p.floor_ulps = floor_ulps;
    p.emd = d_emd; p.iters = d_iters; p.err = d_err; p.flags = d_flags;
    p.track_list = pl->track_list; p.track_count = ctrl + pilot::CTRL_TRACK_LEN;
    p.queue_head = ctrl + pilot::CTRL_HEAD_FAST; p.queue_shards = nullptr;
    p.ring = 0; p.bands = 1;
    p.fb_list = nullptr; p.fb_count = nullptr;
    p.nan_list = pl->nan_list; p.nan_count = ctrl + pilot::CTRL_NAN_LEN;
    p.unequal = ctrl + pilot::CTRL_UNEQUAL;
    p.debug = 0;
    return p;
}

// The passes that plan_grid (sinkhorn_layout.hpp) lays out for this call, launched in order: every decision is taken there, the
// pointers are bound here.
// captured: the call is being recorded into a graph, whose replays have their pointers baked in: it works on block 0 behind its
// caller's memset node over BOTH control blocks, zeroes nothing in its prep kernel, and leaves the parity to its caller, which
// sets it to 1 after every such call and replay -- block 1 is then the zero one, and the next ordinary call zeroes block 0.
int run_grid(int cfg, pilot_ot_plan *pl, const pilot::SinkhornSwitches &sw, const double *d_P, const double *d_M, double reg, int num_iter_max,
             double stop_thr, double tau, int check_period, double floor_ulps, bool sym, int row_begin, int n_rows, int row_step,
             double *d_emd, int *d_iters, double *d_err, int *d_flags, hipStream_t s, bool mixed, bool captured) {
    const int N = pl->N, K = pl->K, RT = (K + 15) / 16;
    const pilot::GridPasses g = pilot::plan_grid(cfg, N, K, n_rows, sym, mixed, pl->max_cost / reg, pl->n_cu, sw);
    if (g.rc != PILOT_OT_OK) return fail(g.rc, "%s", g.msg);
    if (n_rows == 0) return PILOT_OT_OK;
    int *const ctrl = captured ? pl->ctrl : ctrl_block(pl, pl->ctrl_par);
    int *const zero_ctrl = captured ? nullptr : ctrl_spare(pl);
    pilot::GridParams p = call_params(pl, ctrl, n_rows * N, row_begin, row_step, num_iter_max, check_period, stop_thr, tau, floor_ulps, d_emd, d_iters,
                                      d_err, d_flags);
    p.debug = sw.debug;
    int *const lists[] = {pl->order_list, pl->track_list, pl->nan_list + (size_t)N * N};       // (PairList)
    auto slot = [&](int at) { return at == pilot::CTRL_NONE ? nullptr : ctrl + at; };
    if (g.f64.run) { p.fb_list = lists[g.f64.list]; p.fb_count = slot(pilot::CTRL_FB_LEN); }
    if (g.fast.solo_blocks) { p.solo_len = slot(pilot::CTRL_SOLO_LEN); p.solo_head = slot(pilot::CTRL_HEAD_SOLO); }
    auto launch = [&](const pilot::PassPlan &v) -> hipError_t {
        p.list = lists[v.list]; p.list_len = slot(v.len_slot); p.queue_head = slot(v.head_slot); p.queue_shards = slot(v.shards_at);
        p.solo_blocks = v.solo_blocks; p.ring = v.lds.ring; p.bands = v.bands;
        const dim3 wgs(v.wgs);
        if (v.solo_f64) return pilot::launch_solo_track_f64(wgs, s, p);
        if (v.tv) return pilot::launch_stream_tv(v.cfg, v.tv, RT, sym, v.track, wgs, v.lds.bytes, s, p);
        if (v.quad) return pilot::launch_quad(wgs, s, p);
        if (v.cfg == pilot::CFG_H32) return pilot::launch_stream_h32(RT, sym, v.live1, wgs, v.lds.bytes, s, p);
        if (v.cfg == pilot::CFG_S32) return pilot::launch_stream_s32(RT, sym, v.track, v.live1, wgs, v.lds.bytes, s, p);
        return v.cfg == pilot::CFG_F64 ? pilot::launch_stream_f64(RT, sym, v.track, wgs, v.lds.bytes, s, p)
                                       : pilot::launch_stream_f32(RT, sym, v.track, wgs, v.lds.bytes, s, p);
    };
    HIP_TRY(pilot::launch_prep(cfg, d_M, K, RT, reg, pl->img, d_P, pl->p_slot, N, g.write_tail, stop_thr, floor_ulps, n_rows, row_begin, row_step,
                               pl->order_bucket, slot(pilot::CTRL_ORDER_HIST), pl->order_tiles, pl->order_list, slot(pilot::CTRL_SPLIT),
                               slot(pilot::CTRL_HEAD_FAST), g.mode, g.ob, zero_ctrl, s));
    if (!captured) pl->ctrl_par ^= 1;       // (the prep launch is issued: the other block is zero when the next call starts)
    hipEvent_t *ev = (pl->timing > 0 && (pl->n_calls++ % pl->timing) == 0) ? pl->ev[pl->n_timed % TIMING_RING] : nullptr;
    if (ev) HIP_TRY(hipEventRecord(ev[0], s));
    if (g.fast.run) HIP_TRY(launch(g.fast));
    if (ev) HIP_TRY(hipEventRecord(ev[1], s));     // (end of the main pass = begin of the tracking pass: one record)
    // (the fp16-split configuration tracks on the bf16-split operand block behind its own)
    p.img = static_cast<float *>(pl->img) + pilot::track_img_elems(cfg, RT);
    HIP_TRY(launch(g.track));
    if (g.f64.run) {
        HIP_TRY(pilot::launch_prep(pilot::CFG_F64, d_M, K, RT, reg, pl->img, d_P, pl->p_slot, N, 2, stop_thr, floor_ulps, 0, row_begin, row_step,
                                   pl->order_bucket, slot(pilot::CTRL_ORDER_HIST), pl->order_tiles, pl->order_list, slot(pilot::CTRL_SPLIT),
                                   slot(pilot::CTRL_HEAD_FAST), 0, 1, nullptr, s));
        p.img = pl->img; p.fb_list = nullptr; p.fb_count = nullptr;
        HIP_TRY(launch(g.f64));
    }
    if (ev) { HIP_TRY(hipEventRecord(ev[2], s)); ++pl->n_timed; }
    if (sw.debug & pilot::DBG_NO_NAN_PASS) return PILOT_OT_OK;
    return run_generic(pl, sw, d_P, d_M, reg, num_iter_max, stop_thr, tau, check_period, row_begin, n_rows, row_step, d_emd, d_iters, d_err, d_flags,
                       s, ctrl, pl->nan_list, slot(pilot::CTRL_NAN_LEN), slot(pilot::CTRL_NAN_HEAD));
}

// 128 < K <= 256 with a symmetric cost inside the fp16-split range: sinkhorn_wide_kernel (wide_kernels.hpp) on the operand
// block the ordinary prep kernel writes for 16 row-tiles, then the value kernel; hand-overs (tau-absorbing / NaN pairs, or
// every pair when the histograms carry unequal mass) are solved by the POT-literal kernel like those of the stream kernels.
int run_wide(pilot_ot_plan *pl, const pilot::SinkhornSwitches &sw, const double *d_P, const double *d_M, double reg, int num_iter_max, double stop_thr, double tau,
             int check_period, double floor_ulps, int row_begin, int n_rows, int row_step, double *d_emd, int *d_iters, double *d_err,
             int *d_flags, hipStream_t s) {
    const int N = pl->N, K = pl->K, RT = 16;
    // the records are 2 KB per pair: a big grid is solved in row chunks of at most WIDE_CHUNK_PAIRS pairs (1 GB of records),
    // each a complete call of its own (same kernels, same pair -> same bits whatever the chunking)
    long WIDE_CHUNK_PAIRS = 512L * 1024;
    if (const char *e = pilot::test_switch("PILOT_OT_WIDE_CHUNK")) { const long v = atol(e); if (v > 0) WIDE_CHUNK_PAIRS = v; }     // (tests)
    if ((long)n_rows * N > WIDE_CHUNK_PAIRS && n_rows > 1) {
        const int rows_per = (int)(WIDE_CHUNK_PAIRS / N) > 0 ? (int)(WIDE_CHUNK_PAIRS / N) : 1;
        for (int r0 = 0; r0 < n_rows; r0 += rows_per) {
            const int nr = n_rows - r0 < rows_per ? n_rows - r0 : rows_per;
            const size_t off = (size_t)r0 * N;
            const int rc = run_wide(pl, sw, d_P, d_M, reg, num_iter_max, stop_thr, tau, check_period, floor_ulps, row_begin + r0 * row_step, nr, row_step,
                                    d_emd + off, d_iters ? d_iters + off : nullptr, d_err ? d_err + off : nullptr, d_flags + off, s);
            if (rc != PILOT_OT_OK) return rc;
        }
        return PILOT_OT_OK;
    }
    // (this path keeps its memset and block 0: no plan runs both it and run_grid, which is for K <= 128)
    HIP_TRY(hipMemsetAsync(pl->ctrl, 0, (pilot::CTRL_ORDER_HIST + 2 * pilot::ORDER_NB) * sizeof(int), s));
    if (n_rows == 0) return PILOT_OT_OK;
    const int n_pairs = n_rows * N;
    if ((size_t)n_pairs > pl->wide_rec_n) {     // (first call of this size: the one allocation of the path)
        if (pl->wide_rec) HIP_TRY(hipFree(pl->wide_rec));
        pl->wide_rec = nullptr; pl->wide_rec_n = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pl->wide_rec), sizeof(float) * pilot::wide_rec_elems() * (size_t)n_pairs));
        pl->wide_rec_n = (size_t)n_pairs;
    }
    int ob = (n_pairs + 1023) / 1024;
    if (ob > pl->n_cu) ob = pl->n_cu;
    HIP_TRY(pilot::launch_prep(pilot::CFG_H32, d_M, K, RT, reg, pl->img, d_P, pl->p_slot, N, 0, stop_thr, floor_ulps, n_rows, row_begin, row_step,
                               pl->order_bucket, pl->ctrl + pilot::CTRL_ORDER_HIST, pl->order_tiles, pl->order_list, pl->ctrl + pilot::CTRL_SPLIT,
                               pl->ctrl + pilot::CTRL_HEAD_FAST, 0, ob, nullptr, s));
    const pilot::GridParams p = call_params(pl, pl->ctrl, n_pairs, row_begin, row_step, num_iter_max, check_period, stop_thr, tau, floor_ulps, d_emd,
                                            d_iters, d_err, d_flags);
    hipEvent_t *ev = (pl->timing > 0 && (pl->n_calls++ % pl->timing) == 0) ? pl->ev[pl->n_timed % TIMING_RING] : nullptr;
    if (ev) HIP_TRY(hipEventRecord(ev[0], s));
    const int tiles = (n_pairs + 15) / 16;
    int wgs = pl->n_cu < tiles ? pl->n_cu : tiles;            // one 512-thread workgroup per CU (230 VGPRs: two waves per SIMD)
    HIP_TRY(pilot::launch_wide(dim3(wgs), s, p, pl->wide_rec));
    if (ev) HIP_TRY(hipEventRecord(ev[1], s));     // (end of the main pass = begin of the tracking pass: one record)
    HIP_TRY(pilot::launch_wide_value(dim3(pilot::clamp_wgs(pl->n_cu, 2, tiles)), s, p, pl->wide_rec));
    if (ev) { HIP_TRY(hipEventRecord(ev[2], s)); ++pl->n_timed; }
    return run_generic(pl, sw, d_P, d_M, reg, num_iter_max, stop_thr, tau, check_period, row_begin, n_rows, row_step, d_emd, d_iters, d_err,
                       d_flags, s, pl->ctrl, pl->nan_list, pl->ctrl + pilot::CTRL_NAN_LEN, pl->ctrl + pilot::CTRL_NAN_HEAD);
}

pilot::SinkhornSwitches read_switches() {
    const char *dbg = pilot::test_switch("PILOT_OT_DEBUG");       // (a lookup's value lasts until the next lookup)
    const int debug = dbg ? atoi(dbg) : 0;
    const int no_quad = pilot::test_switch("PILOT_OT_NO_QUAD") ? 1 : 0;
    const char *gw = pilot::test_switch("PILOT_OT_GENERIC_WGS");
    return {debug, no_quad, gw ? atoi(gw) : 0};
}

}  // namespace

PILOT_API int pilot_ot_sinkhorn_grid_dev(pilot_ot_plan *pl, const double *d_P, const double *d_M, double reg,
                                         int num_iter_max, double stop_thr, double tau, int check_period,
                                         int precision, double f32_floor_ulps, int cost_is_symmetric,
                                         int row_begin, int row_end, int row_step, double *d_emd, int *d_iters,
                                         double *d_err, int *d_flags, void *stream) {
    if (!pl || !d_P || !d_M || !d_emd) return fail(PILOT_OT_EINVAL, "NULL pointer");
    int rc = check_grid_args(pl->N, pl->K, reg, num_iter_max, stop_thr, tau, check_period, precision, row_begin,
                             row_end, row_step);
    if (rc != PILOT_OT_OK) return rc;
    // the test switches that act inside the launch sequence, read once: every lookup takes a lock, and the graph key holds them
    const pilot::SinkhornSwitches sw = read_switches();
    if (!d_flags) d_flags = pl->flags_ws;
    {
        const int n_rows_g = (row_end - row_begin + row_step - 1) / row_step;
        // K beyond the MFMA kernels, a reg beyond the f64 range of exp(-M/reg) (judged by the plan's max_cost), or on request: POT's loop literally, absorbed kernel rebuilt per pair
        // 128 < K <= 256 (the fixed Gibbs image no longer fits one wave's registers and LDS): eight waves per tile while the
        // call is inside the fp16-split range with a symmetric cost; an explicit f64 / POT-literal request, a non-symmetric cost
        // or a smaller reg keep the POT-literal kernel
        if (pl->K > MAX_K && pl->K <= WIDE_MAX_K && cost_is_symmetric && precision != PILOT_OT_PREC_GENERIC && precision != PILOT_OT_PREC_F64 &&
            pl->max_cost / reg <= h_max_cost_over_reg() && tau <= pilot::H_MAX_TAU && !pilot::test_switch("PILOT_OT_NO_WIDE")) {
            if (!(f32_floor_ulps > 0.0)) f32_floor_ulps = 8.0;
            return run_wide(pl, sw, d_P, d_M, reg, num_iter_max, stop_thr, tau, check_period, f32_floor_ulps, row_begin, n_rows_g, row_step, d_emd,
                            d_iters, d_err, d_flags, static_cast<hipStream_t>(stream));
        }
        if (precision == PILOT_OT_PREC_GENERIC || pl->K > MAX_K || pl->max_cost / reg > MAX_COST_OVER_REG)
            return run_generic(pl, sw, d_P, d_M, reg, num_iter_max, stop_thr, tau, check_period, row_begin, n_rows_g, row_step, d_emd,
                               d_iters, d_err, d_flags, static_cast<hipStream_t>(stream), ctrl_spare(pl));
    }
    // (the range is judged by the plan's max_cost / reg: 1 / reg for Trajectory.py:101's normalised cost unless the caller said
    // otherwise with pilot_ot_plan_set_max_cost; the host and multi-device entry points set it from the M they copy in)
    precision = pilot_ot_resolve_precision(precision, pl->max_cost / reg, pl->K, cost_is_symmetric, tau);
    bool mixed = false;
    if (precision == PILOT_OT_PREC_AUTO_MIXED) {
        precision = PILOT_OT_PREC_F64;
        mixed = true;
    }
    // beyond the f32 range AUTO still tries f32 first, pair by pair, where the split images fit and POT's defaults hold
    mixed = mixed && split_fits_lds(pl->K, cost_is_symmetric != 0, 2) && pl->max_cost / reg <= 140.0 && !pilot::test_switch("PILOT_OT_NO_MIXED");
    if (!(f32_floor_ulps > 0.0)) f32_floor_ulps = 8.0;
    const int n_rows = (row_end - row_begin + row_step - 1) / row_step;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cfg = mixed ? pilot::CFG_S32
                          : (precision == PILOT_OT_PREC_F32 ? pilot::CFG_F32
                             : (precision == PILOT_OT_PREC_BF16X3 ? pilot::CFG_S32 : (precision == PILOT_OT_PREC_F16X2 ? pilot::CFG_H32 : pilot::CFG_F64)));
    auto run = [&](hipStream_t on, bool captured) -> int {
        if (captured) HIP_TRY(hipMemsetAsync(pl->ctrl, 0, 2 * pilot::CTRL_BLOCK_INTS * sizeof(int), on));      // (the graph's memset node)
        int r = run_grid(cfg, pl, sw, d_P, d_M, reg, num_iter_max, stop_thr, tau, check_period, f32_floor_ulps, cost_is_symmetric != 0,
                         row_begin, n_rows, row_step, d_emd, d_iters, d_err, d_flags, on, mixed, captured);
        // a shape whose operand images do not fit LDS in this precision (non-symmetric cost at large K): the POT-literal
        // kernel takes the whole grid -- the reference has no such limit
        if (r == PILOT_OT_ENOTSUP)
            r = run_generic(pl, sw, d_P, d_M, reg, num_iter_max, stop_thr, tau, check_period, row_begin, n_rows, row_step, d_emd, d_iters,
                            d_err, d_flags, on, captured ? pl->ctrl : ctrl_spare(pl));
        return r;
    };
    if (!pl->graph_mode || pl->timing || n_rows == 0) return run(s, false);
    // graph replay: the first call with a new argument set runs as usual (and grows the work buffers), the second one is
    // captured, later ones replay the instantiated graph
    const pilot_ot_plan::GraphKey key = {d_P, d_M, d_emd, d_iters, d_err, d_flags, reg, stop_thr, tau, f32_floor_ulps, pl->max_cost, num_iter_max,
                                         check_period, cfg, mixed ? 1 : 0, cost_is_symmetric != 0 ? 1 : 0, row_begin, n_rows, row_step, sw};
    if (pl->gexec && key == pl->gkey) {
        HIP_TRY(hipGraphLaunch(pl->gexec, s));
        pl->ctrl_par = 1;
        return PILOT_OT_OK;
    }
    if (pl->gexec) { (void)hipGraphExecDestroy(pl->gexec); pl->gexec = nullptr; }
    if (!(pl->gkey_seen && key == pl->gkey)) {
        pl->gkey = key; pl->gkey_seen = 1;
        return run(s, false);
    }
    if (!pl->gstream) HIP_TRY(hipStreamCreateWithFlags(&pl->gstream, hipStreamNonBlocking));
    HIP_TRY(hipStreamBeginCapture(pl->gstream, hipStreamCaptureModeThreadLocal));
    rc = run(pl->gstream, true);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(pl->gstream, &graph);
    if (rc != PILOT_OT_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ce != hipSuccess) { (void)hipGetLastError(); return fail(PILOT_OT_EHIP, "graph capture failed: %s", hipGetErrorString(ce)); }
    const hipError_t ie = hipGraphInstantiate(&pl->gexec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) { (void)hipGetLastError(); pl->gexec = nullptr; return fail(PILOT_OT_EHIP, "graph instantiation failed: %s", hipGetErrorString(ie)); }
    HIP_TRY(hipGraphLaunch(pl->gexec, s));
    pl->ctrl_par = 1;       // (a graph works on block 0 behind a memset of both: see run_grid)
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_plan_enable_graph(pilot_ot_plan *pl, int enable) {
    if (!pl) return fail(PILOT_OT_EINVAL, "plan is NULL");
    pl->graph_mode = enable ? 1 : 0;
    if (!enable) {
        if (pl->gexec) { (void)hipGraphExecDestroy(pl->gexec); pl->gexec = nullptr; }
        pl->gkey_seen = 0;
    }
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_sinkhorn_grid(const double *P, int N, int K, const double *M, double reg, int num_iter_max,
                                     double stop_thr, double tau, int check_period, int precision,
                                     double f32_floor_ulps, int cost_is_symmetric, int row_begin, int row_end,
                                     int row_step, double *emd, int *iters, double *err, int *flags) {
    if (!P || !M || !emd) return fail(PILOT_OT_EINVAL, "NULL pointer");
    int rc = check_grid_args(N, K, reg, num_iter_max, stop_thr, tau, check_period, precision, row_begin, row_end,
                             row_step);
    if (rc != PILOT_OT_OK) return rc;
    double mx = 0.0;
    for (size_t t = 0; t < (size_t)K * K; ++t) mx = M[t] > mx ? M[t] : mx;
    precision = pilot_ot_resolve_precision(precision, mx / reg, K, cost_is_symmetric, tau);     // (max(M) is known here)
    const int n_rows = (row_end - row_begin + row_step - 1) / row_step;
    const size_t n_out = (size_t)n_rows * N;
    if (n_out == 0) return PILOT_OT_OK;

    const bool trace = pilot::test_switch("PILOT_OT_HOST_TRACE") != nullptr;       // (stage stamps on stderr: tools/host_to_host_probe.py)
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    const auto t0 = now();
    rc = pilot::host_ctx_prepare(N, K, n_out);
    if (rc != PILOT_OT_OK) return rc;
    pilot::HostCtx &h = pilot::thread_host();
    hipError_t e = hipMemcpy(h.dP, P, sizeof(double) * (size_t)N * K, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h.dM, M, sizeof(double) * (size_t)K * K, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(PILOT_OT_EHIP, "H2D copy failed: %s", hipGetErrorString(e));
    const auto t1 = now();
    h.plan->max_cost = mx > 0.0 ? mx : 1.0;
    rc = pilot_ot_sinkhorn_grid_dev(h.plan, h.dP, h.dM, reg, num_iter_max, stop_thr, tau, check_period, precision,
                                    f32_floor_ulps, cost_is_symmetric, row_begin, row_end, row_step, h.dE,
                                    iters ? h.dIt : nullptr, err ? h.dErr : nullptr, h.dFl, nullptr);
    if (rc != PILOT_OT_OK) return rc;
    const auto t2 = now();
    if (trace) (void)hipStreamSynchronize(nullptr);
    const auto t3 = now();
    const pilot::Fetch f[4] = {{emd, h.dE, sizeof(double) * n_out}, {iters, h.dIt, sizeof(int) * n_out},
                        {err, h.dErr, sizeof(double) * n_out}, {flags, h.dFl, sizeof(int) * n_out}};
    rc = pilot::host_fetch(f, 4);
    if (trace) fprintf(stderr, "pilot_ot_sinkhorn_grid: prepare + H2D %.0f us, enqueue %.0f us, device %.0f us, fetch %.0f us\n", us(t0, t1), us(t1, t2), us(t2, t3), us(t3, now()));
    return rc;
}

// ------------------------------------------------------------------------------------------------
PILOT_API int pilot_ot_plan_enable_timing(pilot_ot_plan *pl, int enable) {
    if (!pl) return fail(PILOT_OT_EINVAL, "plan is NULL");
    if (enable)
        for (int i = 0; i < TIMING_RING; ++i)
            for (int j = 0; j < 3; ++j)
                if (!pl->ev[i][j]) HIP_TRY(hipEventCreate(&pl->ev[i][j]));
    pl->timing = enable > 0 ? enable : 0;       // n > 1: every n-th call is timed (the event records cost a 0.7 ms call 2 %)
    pl->n_timed = 0; pl->n_calls = 0;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_plan_kernel_times(pilot_ot_plan *pl, int max_n, float *main_ms, float *track_ms, int *n_out) {
    if (!pl || !main_ms || !track_ms || !n_out) return fail(PILOT_OT_EINVAL, "NULL pointer");
    long n = pl->n_timed < TIMING_RING ? pl->n_timed : TIMING_RING;
    if (n > max_n) n = max_n;
    for (long t = 0; t < n; ++t) {
        const long call = pl->n_timed - n + t;
        hipEvent_t *ev = pl->ev[call % TIMING_RING];
        HIP_TRY(hipEventElapsedTime(&main_ms[t], ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&track_ms[t], ev[1], ev[2]));
    }
    *n_out = (int)n;
    return PILOT_OT_OK;
}
