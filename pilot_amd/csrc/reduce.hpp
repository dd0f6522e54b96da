// The fixed-order reductions of the feature kernels, once.  "The same call gives the same bits" rests on every reduction combining
// in one order that depends on nothing but the shape of the workgroup; the orders and the barrier contracts are these and no others.
// `op(a, b)` combines the value held so far (a) with the next one (b); `take(ov, oi, v, i)` replaces the pair (v, i) by (ov, oi)
// when that one is better.  Every thread of the wave / workgroup calls (no divergent call sites); a workgroup is waves of 64 lanes
// along threadIdx.x.
//
// Over the 64 lanes of a wave -- no LDS, no barrier:
//   lanes_reduce(x, op)        xor butterfly, offsets 32, 16, 8, 4, 2, 1: x = op(x, x of lane ^ offset) six times.  Lane l ends with
//                              the tree whose leaves are the lanes in the order l, l^32, l^16, ...; for a commutative op (every use
//                              here) all 64 lanes hold the same bits.  Every lane gets the result.
//   lanes_sum(x)               the same with Sum below.
//   lanes_best(v, i, take)     the same butterfly on a (value, index) pair, in place: take(ov, oi, v, i) with the other lane's pair.
//                              With a total order (ties by index) every lane ends with the same pair.
//
// Over a workgroup of NW waves, wave order -- one barrier (two with the trailing one), NW words of LDS:
//   fold_in_order<NW>(red, op) ((red[0] op red[1]) op red[2]) ... op red[NW-1], from the left, starting AT red[0] (no phantom
//                              zero in front: 0.0 + red[0] differs from red[0] only where red[0] is -0.0, and a wave total whose
//                              per-lane partials started at +0.0 never is, since +0.0 + x is -0.0 for no x and the butterfly adds
//                              such values to each other).  Reads only; the caller has made red[] visible (a barrier since it was
//                              written).
//   waves_in_order<NW>(w, red, op)   w is wave-uniform (a lanes_* result).  Lane 0 of every wave writes red[wave]; barrier;
//                              fold_in_order.  Every thread gets the result.  Before: nobody may still be reading red[0 .. NW) (a
//                              barrier since its last use).  After: red[] is STILL BEING READ -- a barrier before its next write.
//   block_sum<NW> / block_max<NW> (v, red)   lanes_reduce, waves_in_order, then a trailing barrier.  Every thread gets the result.
//                              Before: as waves_in_order.  After: red[] is free the moment the call returns, so calls may follow
//                              each other on one buffer.
//   block_best<NW>(v, i, red_v, red_i, take)   the pair form of the same three steps, in place, with the same contract.
//
// Over a workgroup of NT threads, LDS halving tree -- log2 NT barriers, NT words of LDS; for partials that are in LDS already:
//   tree_fold<NT>(red, op)     for s = NT/2, NT/4, ..., 1: thread t < s does red[t] = op(red[t], red[t + s]); barrier.  In place.
//                              Before: red[0 .. NT) written and made visible (a barrier since).  After: red[0] is the result and
//                              visible to every thread (the last step ends in its barrier); red[1 ..] is scratch; red[] is still
//                              being read -- a barrier before its next write.
//   block_tree_sum<NT>(v, red) red[t] = v; barrier; tree_fold with Sum; read red[0]; trailing barrier.  Every thread gets the
//                              result.  Before: nobody still reading red[].  After: red[] is free the moment the call returns.
//   tree_best<NT>(rv, ri, take)   tree_fold on (value, index) pairs held in two arrays: take(rv[t + s], ri[t + s], rv[t], ri[t]).
//                              Same contract as tree_fold; the result is (rv[0], ri[0]).
//   tree_fold(buf, len, op)    any length, any blockDim: s = the power of two below the first one >= len, then halving; the threads
//                              stride over i < s and do buf[i] = op(buf[i], buf[i + s]) where i + s < len; barrier.  For data that is
//                              its own buffer.  Same contract as tree_fold<NT>.
#pragma once
#include <hip/hip_runtime.h>

namespace pilot {

struct Sum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Max { template <typename T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };     // (a NaN held stays)
// (value, index) orders for the pair forms: the smallest / largest value, the lowest index among equal values
struct LowestMin {
    template <typename T, typename I> __device__ void operator()(T ov, I oi, T &v, I &i) const {
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
};
struct LowestMax {
    template <typename T, typename I> __device__ void operator()(T ov, I oi, T &v, I &i) const {
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
};

template <typename T, typename Op> __device__ inline T lanes_reduce(T x, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(x, off, 64);
        x = op(x, o);
    }
    return x;
}
template <typename T> __device__ inline T lanes_sum(T x) { return lanes_reduce(x, Sum{}); }

template <typename T, typename I, typename Take> __device__ inline void lanes_best(T &v, I &i, Take take) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T ov = __shfl_xor(v, off, 64);
        const I oi = __shfl_xor(i, off, 64);
        take(ov, oi, v, i);
    }
}

template <int NW, typename T, typename Op> __device__ inline T fold_in_order(const T *red, Op op) {
    T r = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r = op(r, red[w]);
    return r;
}
template <int NW, typename T, typename Op> __device__ inline T waves_in_order(T w, T *red, Op op) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    return fold_in_order<NW>(red, op);
}
template <int NW, typename T, typename Op> __device__ inline T block_reduce(T v, T *red, Op op) {
    const T r = waves_in_order<NW>(lanes_reduce(v, op), red, op);
    __syncthreads();
    return r;
}
template <int NW, typename T> __device__ inline T block_sum(T v, T *red) { return block_reduce<NW>(v, red, Sum{}); }
template <int NW, typename T> __device__ inline T block_max(T v, T *red) { return block_reduce<NW>(v, red, Max{}); }

template <int NW, typename T, typename I, typename Take>
__device__ inline void block_best(T &v, I &i, T *red_v, I *red_i, Take take) {
    lanes_best(v, i, take);
    if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = v; red_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = red_v[0]; i = red_i[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) take(red_v[w], red_i[w], v, i);
    __syncthreads();
}

template <int NT, typename T, typename Op> __device__ inline void tree_fold(T *red, Op op) {
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const T o = red[threadIdx.x + s];
            red[threadIdx.x] = op(red[threadIdx.x], o);
        }
        __syncthreads();
    }
}
template <int NT> __device__ inline double block_tree_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    tree_fold<NT>(red, Sum{});
    const double r = red[0];
    __syncthreads();
    return r;
}
template <int NT, typename T, typename I, typename Take> __device__ inline void tree_best(T *rv, I *ri, Take take) {
    const int t = threadIdx.x;
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) take(rv[t + s], ri[t + s], rv[t], ri[t]);
        __syncthreads();
    }
}
template <typename T, typename Op> __device__ inline void tree_fold(T *buf, int len, Op op) {
    int s = 1;
    while (s < len) s <<= 1;
    for (s >>= 1; s > 0; s >>= 1) {
        for (int i = threadIdx.x; i < s; i += blockDim.x)
            if (i + s < len) buf[i] = op(buf[i], buf[i + s]);
        __syncthreads();
    }
}

}  // namespace pilot
