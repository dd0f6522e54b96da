// K21: per selected column of a cells x genes matrix, the tie-averaged ranks of the used rows (code >= 0) summed per group -- the
// one primitive behind the Wilcoxon / Mann-Whitney rank-sum test of every group against the rest (scanpy's
// rank_genes_groups(method="wilcoxon")) and the Kruskal-Wallis test over all groups.  Everything here is an integer:
//   rank2[g][j] = 2 * sum_{i in g} rank_i   (ranks are multiples of 1/2),   ties[j] = sum over runs of equal values of t^3 - t,
// exact for N <= 2^21 - 1 used rows (t^3 fits an int64).  Integer addition has no order, so LDS and global integer atomics are
// used freely and the dense route, the sparse route and a repeated call return the same integers; there is no floating-point
// atomic and no floating-point arithmetic at all on the device.
//
// Only the non-zero values are ever sorted.  The z = N - L zeros of a column (implicit, stored 0.0 or -0.0 alike) are one run that
// sits after the `neg` negative values: each has 2 * rank = 2 * neg + z + 1, positive values are shifted by z, and a group's zeros
// are count[g] minus its non-zero used entries of the column.
//
// Passes (host: pilot_ot_rank_sums.hip):
//   scan<FILL = false>  counts the non-zero used entries L[j] of every selected position j and reports the first non-finite used
//                       value as min((j << 32) | row); an unused row's value is never read.
//   (host)              bins the positions by L and gives each a slice of the record buffer: L records, or the next power of two
//                       for a column of the long bin.
//   scan<FILL = true>   writes the records, one per non-zero used entry, in any order (the slot comes from an integer atomic).
//   rank                one workgroup per column: bitonic sort by value, then every record finds its run [lo, hi) by two binary
//                       searches and adds 2 * (lo + shift) + (hi - lo) + 1 to its group's int64 accumulator in LDS; the run's
//                       first record adds t^3 - t.
// A record is the order-preserving image of the value's bits (sign bit flipped for positives, all bits for negatives; -0 never
// reaches a record) with the group: float32 packs both into 64 bits, float64 takes 16 bytes.
//
// Bins, by L: <= RS_WAVE_MAX one wave per column; <= RS_WG_MAX a workgroup of RS_THREADS with the column in LDS; longer columns
// are sorted in HBM by the same workgroup, every compare-exchange distance below RS_SORT_TILE running on tiles staged in LDS.
// LDS per workgroup: the records (RS_WG_MAX x 8 B = 64 KiB, float64 128 KiB) + 12 B per group + 8, of the CU's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>

namespace pilot {

typedef unsigned long long rs_u64;

constexpr int RS_WAVE_MAX = 64;            // pilot_ot_rank_sums_wave_max
constexpr int RS_WG_MAX = 8192;            // pilot_ot_rank_sums_wg_max
constexpr int RS_SORT_TILE = 8192;         // pilot_ot_rank_sums_sort_tile: the long bin's LDS tile
constexpr int RS_THREADS = 1024;
constexpr int RS_MAX_GROUPS = 1024;
constexpr long long RS_MAX_ROWS = (1LL << 21) - 1;
constexpr int RS_SCAN_ROWS = 1024;         // least rows per workgroup of the dense scan
constexpr rs_u64 RS_NO_BAD = ~0ull;

template <typename T> struct RsKey;
template <> struct RsKey<float> {
    typedef rs_u64 Rec;
    static constexpr rs_u64 ZERO = 0x80000000ull;          // value(+0.0f)
    __device__ static Rec make(float v, int g) {
        unsigned u = __float_as_uint(v);
        u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
        return ((rs_u64)u << 32) | (unsigned)g;
    }
    __device__ static rs_u64 value(Rec r) { return r >> 32; }
    __device__ static int group(Rec r) { return (int)(unsigned)r; }
    __device__ static Rec pad() { return ~0ull; }
};
struct RsRec64 {
    rs_u64 key;
    long long group;
};
template <> struct RsKey<double> {
    typedef RsRec64 Rec;
    static constexpr rs_u64 ZERO = 0x8000000000000000ull;
    __device__ static Rec make(double v, int g) {
        rs_u64 u = (rs_u64)__double_as_longlong(v);
        u ^= (u >> 63) ? ~0ull : 0x8000000000000000ull;
        return Rec{u, g};
    }
    __device__ static rs_u64 value(const Rec &r) { return r.key; }
    __device__ static int group(const Rec &r) { return (int)r.group; }
    __device__ static Rec pad() { return Rec{~0ull, 0}; }
};

// one used entry (row i, group g >= 0, value v) of position j: counted or written
template <typename T, bool FILL>
__device__ inline void rs_visit(T v, int g, int j, long long i, int &cnt, int *len, const long long *off, typename RsKey<T>::Rec *rec,
                                rs_u64 *bad) {
    if (!FILL) {
        if (!__builtin_isfinite(v)) atomicMin(bad, ((rs_u64)(unsigned)j << 32) | (rs_u64)i);
        else if (v != (T)0) ++cnt;
    } else if (v != (T)0) {
        const int slot = atomicAdd(&len[j], 1);
        rec[off[j] + slot] = RsKey<T>::make(v, g);
    }
}

// Dense: a workgroup is 64 positions x 4 row phases over `rows_per` rows; a row's 64 values are adjacent when the columns are.
// len: L[j] (FILL = false: added to; FILL = true: the zeroed cursor).  Grid: (ceil(n_sel / 64), ceil(n / rows_per)).
template <typename T, bool FILL>
__global__ void __launch_bounds__(256) rs_dense_scan_kernel(const T *__restrict__ Y, long long ld, long long n, long long rows_per,
                                                            const int *__restrict__ codes, const int *__restrict__ cols, int n_sel,
                                                            int *len, const long long *__restrict__ off,
                                                            typename RsKey<T>::Rec *rec, rs_u64 *bad) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= n_sel) return;
    const long long c = cols ? cols[j] : j;
    const long long i0 = (long long)blockIdx.y * rows_per, i1 = min(n, i0 + rows_per);
    int cnt = 0;
    for (long long i = i0 + (threadIdx.x >> 6); i < i1; i += 4) {
        const int g = codes[i];
        if (g >= 0) rs_visit<T, FILL>(Y[i * ld + c], g, j, i, cnt, len, off, rec, bad);
    }
    if (!FILL && cnt) atomicAdd(&len[j], cnt);
}

// Sparse, from the column form: one workgroup per selected position.
template <typename T, bool FILL>
__global__ void __launch_bounds__(256) rs_csr_scan_kernel(const long long *__restrict__ colptr, const int *__restrict__ rowidx,
                                                          const T *__restrict__ cdata, const int *__restrict__ codes,
                                                          const int *__restrict__ cols, int *len, const long long *__restrict__ off,
                                                          typename RsKey<T>::Rec *rec, rs_u64 *bad) {
    const int j = blockIdx.x;
    const int c = cols ? cols[j] : j;
    const long long p1 = colptr[c + 1];
    int cnt = 0;
    for (long long p = colptr[c] + threadIdx.x; p < p1; p += 256) {
        const int i = rowidx[p];
        const int g = codes[i];
        if (g >= 0) rs_visit<T, FILL>(cdata[p], g, j, i, cnt, len, off, rec, bad);
    }
    if (!FILL && cnt) atomicAdd(&len[j], cnt);
}

// every compare-exchange distance below `tile` of the merges k_lo .. k_hi on a tile in LDS whose first element is element `base`
// of the whole (ascending) sort; ends on a barrier
template <typename K, int THREADS>
__device__ inline void rs_bitonic_lds(typename K::Rec *s, int tile, long long base, long long k_lo, long long k_hi) {
    for (long long k = k_lo; k <= k_hi; k <<= 1)
        for (int d = (int)min(k >> 1, (long long)(tile >> 1)); d > 0; d >>= 1) {
            for (int t = threadIdx.x; t < (tile >> 1); t += THREADS) {
                const int lo = ((t & ~(d - 1)) << 1) | (t & (d - 1)), hi = lo | d;
                const typename K::Rec x = s[lo], y = s[hi];
                if ((K::value(x) > K::value(y)) == (((base + lo) & k) == 0)) { s[lo] = y; s[hi] = x; }
            }
            __syncthreads();
        }
}

// first position of a[b .. e) whose value is >= v (UPPER: > v)
template <typename K, bool UPPER> __device__ inline int rs_bound(const typename K::Rec *a, int b, int e, rs_u64 v) {
    while (b < e) {
        const int m = b + ((e - b) >> 1);
        const rs_u64 x = K::value(a[m]);
        if (UPPER ? x <= v : x < v) b = m + 1;
        else e = m;
    }
    return b;
}

// list: the positions of this bin; len / off: L[j] and the first record of j; cap: records the LDS buffer holds (a power of two;
// L <= cap, or the long bin with its slice padded to a power of two >= 2 cap).  count[g]: used rows of group g; n_used their sum.
// Dynamic LDS: cap records | n_groups + 1 int64 (the groups' 2 * rank sums, the tie term) | n_groups int (non-zero entries).
template <typename T, int THREADS>
__global__ void __launch_bounds__(THREADS) rs_rank_kernel(const int *__restrict__ list, const int *__restrict__ len,
                                                          const long long *__restrict__ off, typename RsKey<T>::Rec *rec, int cap,
                                                          const long long *__restrict__ count, int n_groups, long long n_used,
                                                          int n_sel, long long *__restrict__ rank2, long long *__restrict__ ties) {
    typedef RsKey<T> K;
    typedef typename K::Rec Rec;
    extern __shared__ __attribute__((aligned(16))) char rs_lds[];
    Rec *s = reinterpret_cast<Rec *>(rs_lds);
    rs_u64 *acc = reinterpret_cast<rs_u64 *>(rs_lds + sizeof(Rec) * (size_t)cap);
    int *nz = reinterpret_cast<int *>(acc + n_groups + 1);
    const int tid = threadIdx.x;
    const int j = list[blockIdx.x];
    const int L = len[j];
    Rec *a = rec + off[j];
    for (int g = tid; g <= n_groups; g += THREADS) acc[g] = 0;
    for (int g = tid; g < n_groups; g += THREADS) nz[g] = 0;
    long long P = 1;
    while (P < L) P <<= 1;
    const Rec *sorted = s;
    if (P <= cap) {
        for (int p = tid; p < (int)P; p += THREADS) s[p] = p < L ? a[p] : K::pad();
        __syncthreads();
        rs_bitonic_lds<K, THREADS>(s, (int)P, 0, 2, P);
    } else {
        for (long long p = L + tid; p < P; p += THREADS) a[p] = K::pad();
        __syncthreads();
        for (long long k = cap; k <= P; k <<= 1) {              // first round: every merge up to a tile; then one merge a round
            for (long long d = k >> 1; d >= cap && k > cap; d >>= 1) {
                for (long long t = tid; t < (P >> 1); t += THREADS) {
                    const long long lo = ((t & ~(d - 1)) << 1) | (t & (d - 1)), hi = lo | d;
                    const Rec x = a[lo], y = a[hi];
                    if ((K::value(x) > K::value(y)) == ((lo & k) == 0)) { a[lo] = y; a[hi] = x; }
                }
                __syncthreads();
            }
            for (long long base = 0; base < P; base += cap) {
                for (int p = tid; p < cap; p += THREADS) s[p] = a[base + p];
                __syncthreads();
                rs_bitonic_lds<K, THREADS>(s, cap, base, k > cap ? k : 2, k);
                for (int p = tid; p < cap; p += THREADS) a[base + p] = s[p];
                __syncthreads();
            }
        }
        sorted = a;
    }
    const long long z = n_used - L;
    long long tie = 0;
    for (int p = tid; p < L; p += THREADS) {
        const Rec r = sorted[p];
        const rs_u64 v = K::value(r);
        const int lo = rs_bound<K, false>(sorted, 0, p, v), hi = rs_bound<K, true>(sorted, p + 1, L, v);
        const long long t = hi - lo;
        const int g = K::group(r);
        atomicAdd(&acc[g], (rs_u64)(2 * (lo + (v > K::ZERO ? z : 0)) + t + 1));
        atomicAdd(&nz[g], 1);
        if (p == lo) tie += t * t * t - t;
    }
    if (tie) atomicAdd(&acc[n_groups], (rs_u64)tie);
    __syncthreads();
    const long long neg = rs_bound<K, false>(sorted, 0, L, K::ZERO);
    const long long zero2 = 2 * neg + z + 1;
    for (int g = tid; g < n_groups; g += THREADS)
        rank2[(long long)g * n_sel + j] = (long long)acc[g] + (count[g] - nz[g]) * zero2;
    if (tid == 0) ties[j] = (long long)acc[n_groups] + (z * z * z - z);
}

}  // namespace pilot
