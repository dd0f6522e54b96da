// libpilot_ot.so -- C ABI over the gfx950 kernels (declared in include/pilot_ot.h).
// Host side of the drop-in boundary for pilotpy/tools/Trajectory.py:441-523.
// There is deliberately no CPU implementation in the library: without a HIP device every compute
// entry point returns PILOT_OT_EHIP.
//
// This file is the runtime core the other translation units share (abi_common.hpp, grid_plan.hpp): errors, test switches,
// device queries, the per-thread workspace pool and host staging, shutdown.  Each feature has its own file: pilot_ot_cost.hip
// (K1), pilot_ot_sinkhorn.hip and pilot_ot_emd.hip (the pair grid), pilot_ot_prepass.hip (K4 / K5), pilot_ot_cellw2.hip, ...
#include <hip/hip_runtime.h>
#include <pthread.h>

#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <new>
#include <vector>

#include "abi_common.hpp"
#include "grid_plan.hpp"

namespace {
thread_local char g_err[512] = "";
}

namespace pilot {
int abi_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace pilot

// ------------------------------------------------------------------------------------------------
// test switches: a process-wide table set through pilot_ot_test_switch (never from the environment)
namespace {
std::mutex g_switch_mutex;
std::map<std::string, std::string> g_switches;
}  // namespace
namespace pilot {
const char *test_switch(const char *name) {
    static thread_local std::string value;                                 // (the caller's copy: another thread may set the switch meanwhile)
    std::lock_guard<std::mutex> l(g_switch_mutex);
    if (g_switches.empty()) return nullptr;
    auto it = g_switches.find(name);
    if (it == g_switches.end()) return nullptr;
    value = it->second;
    return value.c_str();
}
}  // namespace pilot

PILOT_API int pilot_ot_test_switch(const char *name, const char *value) {
    std::lock_guard<std::mutex> l(g_switch_mutex);
    if (!name) { g_switches.clear(); return PILOT_OT_OK; }
    if (value) g_switches[name] = value; else g_switches.erase(name);
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_version(void) { return PILOT_OT_VERSION; }
PILOT_API const char *pilot_ot_last_error(void) { return g_err; }

PILOT_API int pilot_ot_device_count(int *count) {
    if (!count) return fail(PILOT_OT_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count = n;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_get_device(int *device) {
    if (!device) return fail(PILOT_OT_EINVAL, "device is NULL");
    HIP_TRY(hipGetDevice(device));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_device_name(char *buf, int buflen) {
    if (!buf || buflen <= 0) return fail(PILOT_OT_EINVAL, "bad buffer");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, buflen, "%s", prop.gcnArchName);
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_dev_alloc(void **dptr, unsigned long long bytes) {
    if (!dptr) return fail(PILOT_OT_EINVAL, "dptr is NULL");
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));
    return PILOT_OT_OK;
}
PILOT_API int pilot_ot_dev_free(void *dptr) {
    HIP_TRY(hipFree(dptr));
    return PILOT_OT_OK;
}
PILOT_API int pilot_ot_memcpy_h2d(void *dst, const void *src, unsigned long long bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return PILOT_OT_OK;
}
PILOT_API int pilot_ot_memcpy_d2h(void *dst, const void *src, unsigned long long bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}
PILOT_API int pilot_ot_stream_sync(void *stream) {
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return PILOT_OT_OK;
}

// ------------------------------------------------------------------------------------------------
namespace {
// Temporaries of the host entry points come from a per-thread pool that only grows (hipMalloc / hipFree cost about a
// millisecond a pair and hipFree synchronises the device: nine of them were most of a 22 ms medians call); released by
// pilot_ot_shutdown().  One buffer per pilot::WsSlot.  A hand-out is an undefined buffer (abi_common.hpp, ws_buffer): under the test
// switch PILOT_OT_WS_GUARD it is poisoned and followed by a canary, so a kernel that reads what nobody wrote or touches the slack
// shows (tests/test_gpu_ws_guard.py); with the switch unset get() makes the HIP calls it always made.
struct WsPool {
    static constexpr int SLOTS = pilot::WS_SLOTS;
    static constexpr size_t GUARD_SLACK = 256;            // least canary bytes behind a guarded request
    static constexpr int POISON = 0xFF, CANARY = 0xA5;
    void *p[SLOTS] = {};
    size_t cap[SLOTS] = {};
    int device = -1;
    // guard mode (test switch PILOT_OT_WS_GUARD): request of each slot's last guarded hand-out, the slots handed out under guard since
    // the last reset, and the earliest canary damage found since then
    size_t req[SLOTS] = {};
    bool guarded[SLOTS] = {};
    unsigned char seen[SLOTS] = {};
    int bad_slot = -1;
    long long bad_offset = 0, bad_request = 0;
    bool selftest_done = false;
    void release() {
        for (int i = 0; i < SLOTS; ++i) { if (p[i]) (void)hipFree(p[i]); p[i] = nullptr; cap[i] = 0; guarded[i] = false; }
        device = -1;
    }
    hipError_t grow(int slot, size_t bytes) {
        if (p[slot]) (void)hipFree(p[slot]);
        p[slot] = nullptr; cap[slot] = 0; guarded[slot] = false;
        const size_t want = bytes + bytes / 4 + 256;
        const hipError_t e = hipMalloc(&p[slot], want);
        if (e == hipSuccess) cap[slot] = want;
        return e;
    }
    // the canary [req, cap) of a guarded slot, read back; the device must be idle
    hipError_t check_canary(int slot) {
        if (!guarded[slot] || !p[slot]) return hipSuccess;
        const size_t n = cap[slot] - req[slot];
        std::vector<unsigned char> h(n);
        const hipError_t e = hipMemcpy(h.data(), static_cast<unsigned char *>(p[slot]) + req[slot], n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        for (size_t i = 0; i < n && bad_slot < 0; ++i)
            if (h[i] != (unsigned char)CANARY) { bad_slot = slot; bad_offset = (long long)i; bad_request = (long long)req[slot]; }
        return hipSuccess;
    }
    hipError_t get_guarded(int slot, size_t bytes, void **out, bool selftest) {
        hipError_t e = hipDeviceSynchronize();       // (entry points launch on streams that do not order against the null stream)
        if (e == hipSuccess) e = check_canary(slot);
        if (e == hipSuccess && bytes + GUARD_SLACK > cap[slot]) e = grow(slot, bytes);
        unsigned char *b = static_cast<unsigned char *>(p[slot]);
        if (e == hipSuccess) e = hipMemset(b, POISON, bytes);
        if (e == hipSuccess) e = hipMemset(b + bytes, CANARY, cap[slot] - bytes);
        if (e == hipSuccess && selftest && !selftest_done) {       // the control: one damaged byte inside the slot's own slack
            selftest_done = true;
            e = hipMemset(b + bytes + 7, 0, 1);
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return e;
        req[slot] = bytes; guarded[slot] = true; seen[slot] = 1;
        *out = b;
        return hipSuccess;
    }
    hipError_t get(int slot, size_t bytes, void **out) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev != device) { release(); device = dev; }
        if (const char *g = pilot::test_switch("PILOT_OT_WS_GUARD")) {
            const bool selftest = !strcmp(g, "selftest");
            if (selftest || !strcmp(g, "1")) return get_guarded(slot, bytes, out, selftest);
        }
        guarded[slot] = false;                       // (a plain hand-out may use the bytes a canary stood in)
        if (bytes > cap[slot]) {
            e = grow(slot, bytes);
            if (e != hipSuccess) return e;
        }
        *out = p[slot];
        return hipSuccess;
    }
    int report(unsigned char *seen_out, int *slot, long long *offset, long long *request, int reset) {
        bool any = false;
        for (int i = 0; i < SLOTS; ++i) any = any || (guarded[i] && p[i]);
        if (any) {
            HIP_TRY(hipDeviceSynchronize());
            for (int i = 0; i < SLOTS; ++i) HIP_TRY(check_canary(i));
        }
        if (seen_out) memcpy(seen_out, seen, SLOTS);
        if (slot) *slot = bad_slot;
        if (offset) *offset = bad_slot < 0 ? 0 : bad_offset;
        if (request) *request = bad_slot < 0 ? 0 : bad_request;
        if (reset) {                                 // (every canary was just judged: a reported damage is not found again at the next hand-out)
            for (int i = 0; i < SLOTS; ++i) { seen[i] = 0; guarded[i] = false; }
            bad_slot = -1; bad_offset = bad_request = 0; selftest_done = false;
        }
        return PILOT_OT_OK;
    }
};
// Per-thread caches (host-entry workspace + pre-pass pool) live in a process-wide registry, not in thread_local objects:
// pilot_ot_shutdown() releases the caches of EVERY thread (it must not run concurrently with other calls), and the caches
// of a thread that has exited are released by the next thread that creates its own -- never from a thread-exit or
// process-exit hook, where the HIP runtime may already be gone.
struct ThreadCtx { pilot::HostCtx host; WsPool ws; pilot::PrepassClock clock; bool orphan = false; };
std::mutex g_tctx_mutex;
std::vector<ThreadCtx *> g_tctx_all;
struct TctxOwner {
    ThreadCtx *c = nullptr;
    ~TctxOwner() {
        if (!c) return;
        std::lock_guard<std::mutex> l(g_tctx_mutex);
        c->orphan = true;           // (no HIP calls here)
    }
};
thread_local TctxOwner g_tctx_owner;
ThreadCtx &tctx() {
    if (!g_tctx_owner.c) {
        std::lock_guard<std::mutex> l(g_tctx_mutex);
        for (size_t i = 0; i < g_tctx_all.size();) {
            if (g_tctx_all[i]->orphan) {
                g_tctx_all[i]->host.release();
                g_tctx_all[i]->ws.release();
                g_tctx_all[i]->clock.release();
                delete g_tctx_all[i];
                g_tctx_all.erase(g_tctx_all.begin() + (long)i);
            } else {
                ++i;
            }
        }
        g_tctx_owner.c = new ThreadCtx();
        g_tctx_all.push_back(g_tctx_owner.c);
    }
    return *g_tctx_owner.c;
}
}  // namespace

namespace pilot {
HostCtx &thread_host() { return tctx().host; }
PrepassClock &thread_clock() { return tctx().clock; }
hipError_t ws_buffer(WsSlot slot, size_t bytes, void **out) { return tctx().ws.get(slot, bytes, out); }

int cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
    return n;
}

int check_dtype(int dtype) {
    return dtype == 0 || dtype == 1 ? PILOT_OT_OK : fail(PILOT_OT_EINVAL, "dtype=%d must be 0 (float32) or 1 (float64)", dtype);
}

int check_ld(long long ld, int n_cols) {
    return ld >= n_cols ? PILOT_OT_OK : fail(PILOT_OT_EINVAL, "ld=%lld is smaller than n_cols=%d", ld, n_cols);
}

int check_cols(const int *cols, int n_sel, int n_cols) {
    if (n_sel < 0 || (!cols && n_sel != n_cols))
        return fail(PILOT_OT_EINVAL, "n_sel=%d columns selected (without cols it must be all n_cols=%d)", n_sel, n_cols);
    for (int j = 0; cols && j < n_sel; ++j)
        if (cols[j] < 0 || cols[j] >= n_cols) return fail(PILOT_OT_EINVAL, "cols[%d]=%d outside [0, %d)", j, cols[j], n_cols);
    return PILOT_OT_OK;
}

int stage_dense(const void *Y, int is_device, size_t es, long long rows, long long n_cols, long long ld, WsSlot slot, const void **ptr,
                long long *ld_out) {
    if (is_device) { *ptr = Y; *ld_out = ld; return PILOT_OT_OK; }
    unsigned char *d;
    HIP_TRY(ws(slot, (size_t)(rows > 0 ? rows : 1) * n_cols * es, &d));
    if (rows > 0)
        HIP_TRY(hipMemcpy2D(d, (size_t)n_cols * es, Y, (size_t)ld * es, (size_t)n_cols * es, (size_t)rows, hipMemcpyHostToDevice));
    *ptr = d;
    *ld_out = n_cols;
    return PILOT_OT_OK;
}

int stage_f64(const double *src, int is_device, size_t count, WsSlot slot, const double **out) {
    if (is_device) { *out = src; return PILOT_OT_OK; }
    double *d;
    HIP_TRY(ws(slot, count, &d));
    HIP_TRY(hipMemcpy(d, src, sizeof(double) * count, hipMemcpyHostToDevice));
    *out = d;
    return PILOT_OT_OK;
}

int host_ctx_prepare(int N, int K, size_t n_out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HostCtx &h = thread_host();
    if (h.plan && (h.N != N || h.K != K || h.device != dev)) h.release();
    if (!h.plan) {
        int rc = pilot_ot_plan_create(N, K, &h.plan);
        if (rc != PILOT_OT_OK) return rc;
        h.N = N; h.K = K; h.device = dev;
        hipError_t e = hipMalloc(&h.dP, sizeof(double) * (size_t)N * K);
        if (e == hipSuccess) e = hipMalloc(&h.dM, sizeof(double) * (size_t)K * K);
        if (e != hipSuccess) { h.release(); return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e)); }
    }
    if (n_out > h.n_out) {
        if (h.dE) (void)hipFree(h.dE);
        if (h.dErr) (void)hipFree(h.dErr);
        if (h.dIt) (void)hipFree(h.dIt);
        if (h.dFl) (void)hipFree(h.dFl);
        h.dE = h.dErr = nullptr; h.dIt = h.dFl = nullptr; h.n_out = 0;
        hipError_t e = hipMalloc(&h.dE, sizeof(double) * n_out);
        if (e == hipSuccess) e = hipMalloc(&h.dErr, sizeof(double) * n_out);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h.dIt), sizeof(int) * n_out);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h.dFl), sizeof(int) * n_out);
        if (e != hipSuccess) { h.release(); return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e)); }
        h.n_out = n_out;
    }
    const size_t need = n_out * (2 * sizeof(double) + 2 * sizeof(int)) + 4 * 64;
    if (need > h.pin_bytes) {
        if (h.pin) (void)hipHostFree(h.pin);
        h.pin = nullptr; h.pin_bytes = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&h.pin), need, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            h.pin = nullptr;               // no pinned memory: fall back to direct copies
        } else {
            h.pin_bytes = need;
        }
    }
    return PILOT_OT_OK;
}
}  // namespace pilot

namespace {
// Copies out of the pinned block on a few persistent helper threads (host memory only: they make no HIP call).  One thread moves
// a 2.9 MB matrix into the caller's pageable array at 12 - 17 GB/s, 0.2 of the 0.95 ms of a c3 call through the host entry; a thread
// per call costs more than it saves (thread start + the runtime's per-thread set-up: measured, with a 7 ms outlier).  The pool is
// created by the first large fetch of the process, never destroyed (its threads sleep on a condition variable until the process
// ends), and forgotten by a forked child (pthread_atfork), which copies on its own thread.
struct CopyJob { void *dst; const void *src; size_t bytes; int *left; };      // left: jobs of the caller's batch still to finish (guarded by the pool's mutex)
class CopyPool {
public:
    static constexpr int HELPERS = 2;
    static CopyPool *get() {
        static std::once_flag once;
        std::call_once(once, [] {
            g_pool = new (std::nothrow) CopyPool();
            pthread_atfork(nullptr, nullptr, [] { g_pool = nullptr; });      // (the child has no helper threads)
        });
        return g_pool;
    }
    void push(void *dst, const void *src, size_t bytes, int *left) {       // never blocks
        { std::lock_guard<std::mutex> l(m_); ++*left; q_.push_back(CopyJob{dst, src, bytes, left}); }
        cv_.notify_one();
    }
    // the caller's thread copies too (any queued job, its own batch's or another caller's) until its own batch is done
    void finish(int *left) {
        std::unique_lock<std::mutex> l(m_);
        while (*left > 0) {
            if (!q_.empty()) run_one(l);
            else done_.wait(l);
        }
    }
    int helpers() const { return n_started_; }
private:
    CopyPool() {
        for (int t = 0; t < HELPERS; ++t) {
            try { std::thread([this] { loop(); }).detach(); ++n_started_; }
            catch (...) { break; }
        }
    }
    void run_one(std::unique_lock<std::mutex> &l) {
        const CopyJob j = q_.back(); q_.pop_back();
        l.unlock();
        memcpy(j.dst, j.src, j.bytes);
        l.lock();
        if (--*j.left == 0) done_.notify_all();
    }
    void loop() {
        std::unique_lock<std::mutex> l(m_);
        for (;;) {
            cv_.wait(l, [this] { return !q_.empty(); });
            run_one(l);
        }
    }
    static CopyPool *g_pool;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::vector<CopyJob> q_;
    int n_started_ = 0;
};
CopyPool *CopyPool::g_pool = nullptr;
}  // namespace

namespace pilot {
// Small results: one stream sync, then the copies out of the block.  From 1 MB on (a 600 x 600 matrix is 2.9 MB) the transfer is
// cut into a few pieces with an event behind each, and every piece that has landed is copied out by the helper threads (and this
// one) while the next is in flight.
int host_fetch(const Fetch *f, int n) {
    HostCtx &h = thread_host();
    if (!h.pin) {
        HIP_TRY(hipStreamSynchronize(nullptr));
        for (int i = 0; i < n; ++i)
            if (f[i].dst) HIP_TRY(hipMemcpy(f[i].dst, f[i].src, f[i].bytes, hipMemcpyDeviceToHost));
        return PILOT_OT_OK;
    }
    size_t total = 0;
    for (int i = 0; i < n; ++i) if (f[i].dst) total += f[i].bytes;
    constexpr size_t PIPELINE_FROM = (size_t)1 << 20;
    int want_threads = 1 + CopyPool::HELPERS;
    if (const char *e = pilot::test_switch("PILOT_OT_FETCH_THREADS")) { const int w = atoi(e); if (w >= 1 && w < want_threads) want_threads = w; }   // experiment switch
    CopyPool *pool = (total >= PIPELINE_FROM && want_threads > 1) ? CopyPool::get() : nullptr;
    if (!pool || pool->helpers() == 0) {
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            if (!f[i].dst) continue;
            HIP_TRY(hipMemcpyAsync(h.pin + off, f[i].src, f[i].bytes, hipMemcpyDeviceToHost, nullptr));
            off += (f[i].bytes + 63) & ~(size_t)63;
        }
        HIP_TRY(hipStreamSynchronize(nullptr));
        off = 0;
        for (int i = 0; i < n; ++i) {
            if (!f[i].dst) continue;
            memcpy(f[i].dst, h.pin + off, f[i].bytes);
            off += (f[i].bytes + 63) & ~(size_t)63;
        }
        return PILOT_OT_OK;
    }
    while (h.n_fev < HostCtx::FETCH_EVENTS) {
        HIP_TRY(hipEventCreateWithFlags(&h.fev[h.n_fev], hipEventDisableTiming));
        ++h.n_fev;
    }
    struct Piece { unsigned char *dst; const unsigned char *pin; size_t bytes; };
    Piece pieces[HostCtx::FETCH_EVENTS];
    int n_pieces = 0;
    // pieces of >= 768 KB (every hipMemcpyAsync + hipEventRecord pair is ~10 us of this thread), at most as many as there are events
    size_t piece = (size_t)768 << 10;
    while ((total + piece - 1) / piece + (size_t)n > (size_t)HostCtx::FETCH_EVENTS) piece *= 2;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (!f[i].dst) continue;
        for (size_t o = 0; o < f[i].bytes; o += piece) {
            const size_t b = f[i].bytes - o < piece ? f[i].bytes - o : piece;
            HIP_TRY(hipMemcpyAsync(h.pin + off + o, static_cast<const unsigned char *>(f[i].src) + o, b, hipMemcpyDeviceToHost, nullptr));
            HIP_TRY(hipEventRecord(h.fev[n_pieces], nullptr));
            pieces[n_pieces++] = Piece{static_cast<unsigned char *>(f[i].dst) + o, h.pin + off + o, b};
        }
        off += (f[i].bytes + 63) & ~(size_t)63;
    }
    hipError_t err = hipSuccess;
    int left = 0;
    for (int i = 0; i < n_pieces && err == hipSuccess; ++i) {
        err = hipEventSynchronize(h.fev[i]);
        if (err != hipSuccess) break;
        // a landed piece goes to the pool in `want_threads` parts (this thread takes its share in finish())
        const size_t part = ((pieces[i].bytes + want_threads - 1) / want_threads + 4095) & ~(size_t)4095;
        for (size_t o = 0; o < pieces[i].bytes; o += part)
            pool->push(pieces[i].dst + o, pieces[i].pin + o, pieces[i].bytes - o < part ? pieces[i].bytes - o : part, &left);
    }
    pool->finish(&left);
    if (err != hipSuccess) return pilot::abi_fail(PILOT_OT_EHIP, "fetching the results failed: %s", hipGetErrorString(err));
    return PILOT_OT_OK;
}
}  // namespace pilot

namespace {
const char *const g_ws_slot_names[] = {
#define PILOT_WS_SLOT_NAME(name) #name,
    PILOT_WS_SLOT_LIST(PILOT_WS_SLOT_NAME)
#undef PILOT_WS_SLOT_NAME
};
static_assert(sizeof(g_ws_slot_names) / sizeof(g_ws_slot_names[0]) == pilot::WS_SLOTS, "one name per slot");
}  // namespace

PILOT_API int pilot_ot_ws_slot_count(void) { return pilot::WS_SLOTS; }
PILOT_API const char *pilot_ot_ws_slot_name(int slot) { return slot >= 0 && slot < pilot::WS_SLOTS ? g_ws_slot_names[slot] : nullptr; }
PILOT_API int pilot_ot_ws_guard_report(unsigned char *seen, int *bad_slot, long long *bad_offset, long long *bad_request, int reset) {
    return tctx().ws.report(seen, bad_slot, bad_offset, bad_request, reset);
}

PILOT_API int pilot_ot_shutdown(void) {
    {
        std::lock_guard<std::mutex> l(g_tctx_mutex);
        for (ThreadCtx *c : g_tctx_all) { c->host.release(); c->ws.release(); c->clock.release(); }
    }
    pilot::abi_multi_release();
    return PILOT_OT_OK;
}
