// What the Sinkhorn kernels that spread a 16-pair tile over the waves of one workgroup share: sinkhorn_quad_kernel (112 < K <= 128,
// four waves, quad_kernels.hpp) and sinkhorn_wide_kernel (128 < K <= 256, eight waves, wide_kernels.hpp).  Included by those two only.
//
// The formulation is the fp16-split one of sinkhorn_stream_kernel<CfgH32x16, ...> (same scaled domain, stopping rule -- f32 floor of the
// threshold -- and tolerance), with the cell types of a tile spread over the waves: wave w owns the OUTPUT row-tiles 2 w and 2 w + 1.
//   * Its rows of the operand image live in REGISTERS, loaded once per wave; G^T = G (symmetric cost) serves both products, so nothing
//     but panels moves in the update loop.
//   * The accumulator registers of tiles 2 w, 2 w + 1 are exactly k-block w of the next product's B operand (the layout rule of the
//     stream kernel), so after the element-wise step a wave publishes ONE k-block of packed pieces (2 KB) in LDS and reads all of
//     them: two workgroup barriers per update.
//   * Control state (the batch, the columns' pairs, counters, flags) is replicated in every wave and moves only on values every wave
//     reads identically from LDS: the tau flags of the columns (ovc) and the waves' partial squared errors added in wave order.  So the
//     waves never diverge, and as a column's arithmetic sees no other column, a pair's bits do not depend on its slot, its workgroup or
//     the row subset of the call.
// Kernel-specific, on purpose (each is one kernel's code as the compiler sees it): the products (the MFMA order is the bits), the image
// loads, the padding representation, a new pair's initial values, where a hand-over goes and how a finished pair retires.  The tau test
// and its flag protocol around the two barriers are four one-line statements interleaved with those; they stay inline in both kernels.
#pragma once
#include "sinkhorn_kernels.hpp"

namespace pilot {

// Workgroup barrier for data that travels through LDS only.  __syncthreads() also waits for the wave's outstanding GLOBAL stores
// (s_waitcnt vmcnt(0): the outputs of finished pairs, a microsecond or two until L2 acknowledges them) -- in a kernel that meets at
// two barriers per update and writes outputs now and then that wait was 6 us per cost flush (K = 128 at N = 600: 1.58 ms with
// __syncthreads, see profiles/r06/ab_experiments.md).  Nothing the waves of a workgroup tell each other here goes through global memory.
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The batch of TILE consecutive work items a tile draws from: lane % TILE holds one item's pair number and patient rows, and the
// columns that ask for a pair are dealt the next items in column order.
template <int TILE>
struct PairBatch {
    int next = 0, end = 0, base = 0, q = 0, i = 0, j = 0;
    bool exhausted = false;
    struct Deal { bool take; int q, i, j; };

    __device__ __forceinline__ bool empty() const { return next >= end && !exhausted; }
    // the batch at work-list position b (at or past n_items: no work left); one list load and one division per lane and batch
    __device__ __forceinline__ void open(int b, int n_items, const GridParams &p, int col) {
        exhausted = b >= n_items;
        next = exhausted ? n_items : b;
        end = (b + TILE < n_items) ? b + TILE : n_items;
        if (exhausted) end = n_items;
        base = b;
        const int bi = b + col;
        q = (p.list && bi < n_items) ? p.list[bi] : bi;
        const int qv = bi < n_items ? q : 0;
        i = p.row_begin + (qv / p.N) * p.row_step;
        j = qv % p.N;
    }
    // wmask: the columns that want a pair.  take: this column got one (every lane takes part in the permutes)
    __device__ __forceinline__ Deal deal(bool want, unsigned long long wmask, int col) {
        const int avail = end - next;
        const int n_want = (int)__popcll(wmask);
        const int rank = (int)__popcll(wmask & ((1ull << col) - 1ull));
        const int bsel = 4 * ((next + rank - base) & (TILE - 1));
        const Deal d = {want && rank < avail, __builtin_amdgcn_ds_bpermute(bsel, q), __builtin_amdgcn_ds_bpermute(bsel, i),
                        __builtin_amdgcn_ds_bpermute(bsel, j)};
        next = __builtin_amdgcn_readfirstlane(next + (n_want < avail ? n_want : avail));
        return d;
    }
};

// Work-list position of the workgroup's next batch.  The first is the workgroup's own number: no atomic, no barrier.  The later ones
// come from the device-wide counter, behind the statically dealt part; thread 0 draws, the others read it from sh_base (two slots,
// by draw parity: a draw never overwrites what a slower wave has yet to read).
template <int TILE, typename Barrier>
__device__ __forceinline__ int split_draw(int &draws, int (&sh_base)[2], const GridParams &p, Barrier barrier) {
    int base;
    if (draws == 0) {
        base = (int)blockIdx.x * TILE;
    } else {
        if (threadIdx.x == 0)
            sh_base[draws & 1] = (int)gridDim.x * TILE + __hip_atomic_fetch_add(p.queue_head, TILE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        barrier();
        base = __builtin_amdgcn_readfirstlane(sh_base[draws & 1]);
    }
    ++draws;
    return base;
}

// X (my two tiles) -> the packed pieces of my k-block
template <typename C>
__device__ __forceinline__ void split_pieces_of(const typename C::acc_t (&X)[2], u32x4_t &hi, u32x4_t &lo) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        unsigned int a, b;
        quot_pieces(X[h / 2][2 * (h & 1)], X[h / 2][2 * (h & 1) + 1], a, b);
        hi[h] = a; lo[h] = b;
    }
}

// |v o (G^T u) - b| of every column: the waves' partial squared sums meet in red and are added in wave order -- the same sum in every wave
template <typename C, int NWAVES, typename Barrier>
__device__ __forceinline__ float split_marginal_error(const typename C::acc_t (&V)[2], const typename C::acc_t (&ACC)[2],
                                                       const typename C::acc_t (&B)[2], float (&red)[NWAVES][C::TILE], int wave, int col,
                                                       int grp, Barrier barrier) {
    float e2 = 0.f;
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
        float et = 0.f;
#pragma unroll
        for (int r = 0; r < C::NREG; ++r) { const float d = V[tl][r] * ACC[tl][r] - B[tl][r]; et += d * d; }
        e2 += et;
    }
    e2 = group_sum<C>(e2);
    if (grp == 0) red[wave][col] = e2;
    barrier();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) tot += red[w][col];
    return sqrtf(tot);
}

// The stop rule on the error e of a column: a pair whose check is pending ends converged or as NaN, a capped one ends as it is.
__device__ __forceinline__ bool split_stop(float e, bool pending, bool capped, float thr, float &errv, int &flags) {
    bool fin = capped;
    if (pending) {
        errv = e;
        if (e <= thr) { fin = true; flags |= FLAG_CONVERGED; }
        else if (e != e) { fin = true; flags |= FLAG_NAN; }
    }
    return fin;
}

}  // namespace pilot
