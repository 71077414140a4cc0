// Wave64 and block-level building blocks of the kernels (gfx950: a wavefront is 64 lanes, nothing here is portable).
// Every function is called by whole wavefronts; the block-level ones by every thread of the block.
#pragma once
#include <hip/hip_runtime.h>

// The value of lane + d / lane - d (the own value where there is no such lane).  A kernel file may overload these for
// a struct of its own, member by member; the templates below then carry it.
template <typename T>
__device__ __forceinline__ T wave_down(T v, int d) {
    return __shfl_down(v, d, 64);
}
template <typename T>
__device__ __forceinline__ T wave_up(T v, int d) {
    return __shfl_up(v, d, 64);
}

struct WaveAdd {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const {
        return a + b;
    }
};

// Lane 0 receives op over the wavefront: v = op(v, the value of lane + d), d = 32 .. 1.  One tree, one operand order --
// a floating-point call site has the same bits wherever it is written.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, wave_down(v, d));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    return wave_reduce(v, WaveAdd());
}

// Every lane receives op over the wavefront, with the same bits: both operands of every step are exchanged.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_all(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

// Inclusive scan in lane order (Hillis-Steele): v = op(v, the value of lane - d), d = 1 .. 32.  reverse: from lane 63
// down, with lane + d.
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, Op op, bool reverse = false) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = reverse ? wave_down(v, d) : wave_up(v, d);
        if (reverse ? lane + d < 64 : lane >= d) v = op(v, o);
    }
    return v;
}

// the number of set bits of a ballot below my lane: my rank among the lanes that voted
__device__ __forceinline__ int wave_rank(unsigned long long bits) {
    return __popcll(bits & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// wave_count[k] = what wavefront k of the block counted, published by a barrier: the sum of the wavefronts before mine
// and the block's total
template <int WAVES>
__device__ __forceinline__ void waves_before(const int* wave_count, int& before, int& all) {
    const int wv = threadIdx.x >> 6;
    before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        const int c = wave_count[k];
        if (k < wv) before += c;
        all += c;
    }
}

// Exclusive offsets of the threads with `pred` in thread order: returns the rank inside the wavefront, `before` the
// hits of the wavefronts below mine, `all` the block's.  wave_count is WAVES words of LDS; a caller that comes back
// with the next strip puts a barrier behind its last use of before / all.  (A kernel that ranks two predicates behind
// ONE barrier writes the two ballots out itself and calls waves_before / wave_rank twice.)
template <int WAVES>
__device__ __forceinline__ int block_offsets(bool pred, int* wave_count, int& before, int& all) {
    const unsigned long long bits = __ballot(pred);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(bits);
    __syncthreads();
    waves_before<WAVES>(wave_count, before, all);
    return wave_rank(bits);
}

// Sum over a block of 256 threads, returned to thread 0 (0 elsewhere): the shuffle tree, then the four wavefronts in
// order through sh[4].  (The tree of wave_sum written out: through the template the loss kernels of gan.hip and
// elementwise.hip come out with other registers, and they are kept instruction for instruction.)
__device__ __forceinline__ float block_sum_256(float v, float* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    float t = 0.0f;
    if (threadIdx.x == 0) t = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return t;
}
