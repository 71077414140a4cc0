// Tensor summaries on the device (include/hypel.h, hypel_tensor_summary_f32): TensorFlow's histogram::Histogram of many
// float32 tensors that are segments of one buffer, in one call, where the variables live.
//
//   * summary_plan_kernel  : prefix sum of the segments' slice counts (a slice = HYPEL_SUMMARY_SLICE elements)
//   * summary_slice_kernel : one block per slice.  Every element is read once (float4 where the address allows).  Its
//                            bucket is estimated from log2|v| and corrected against the limits around the estimate, so
//                            the table decides: the limits are kept in LDS rounded UP to float32, which compares
//                            against a float32 element exactly as the double does (no float lies between a limit and
//                            its round-up).  Counts go to one LDS histogram per block with integer atomics -- a
//                            wavefront whose lanes all hit one bucket adds its lane count once -- and only the
//                            non-zero counters are flushed, with integer atomics on the int64 output.  min / max /
//                            num / sum / sum_squares leave the block as one partial record per slice.
//   * summary_final_kernel : one block per segment sums its slices' records in a fixed order.
// Integer atomics only: counts are exact and the fp64 sums have one order, so two calls give identical bits.
#include <float.h>
#include <math.h>

#include "common.h"
#include "wave.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int64_t SLICE = HYPEL_SUMMARY_SLICE;
constexpr int MAXL = HYPEL_SUMMARY_MAX_LIMITS;

struct Partial {  // 6 x 8 bytes: HYPEL_SUMMARY_WS_DOUBLES
    double mn, mx, sum, sq;
    int64_t num, bad;
};

__device__ __forceinline__ int64_t slices_of(int64_t size) { return size > 0 ? (size + SLICE - 1) / SLICE : 0; }

__global__ void summary_plan_kernel(const int64_t* __restrict__ table, int n_segs, int64_t* __restrict__ prefix) {
    __shared__ int64_t part[THREADS];
    const int t = threadIdx.x;
    const int64_t per = ((int64_t)n_segs + THREADS - 1) / THREADS;
    const int64_t lo = min(t * per, (int64_t)n_segs), hi = min(lo + per, (int64_t)n_segs);
    int64_t c = 0;
    for (int64_t s = lo; s < hi; ++s) c += slices_of(table[2 * s + 1]);
    part[t] = c;
    __syncthreads();
    if (t == 0) {
        int64_t acc = 0;
        for (int k = 0; k < THREADS; ++k) {
            const int64_t v = part[k];
            part[k] = acc;
            acc += v;
        }
        prefix[n_segs] = acc;
    }
    __syncthreads();
    c = part[t];
    for (int64_t s = lo; s < hi; ++s) {
        prefix[s] = c;
        c += slices_of(table[2 * s + 1]);
    }
}

// upper_bound(limits, v) clamped to n - 1, for a finite v; flim[i] = limits[i] rounded up to float32
__device__ __forceinline__ int bucket_of(const float* flim, int n, int mid, float v) {
    const float a = fabsf(v);
    int idx;
    if (a >= 1e-12f) {  // TensorFlow's table: limits[mid + 1 + k] = 1e-12 * 1.1^k, limits[mid - 1 - k] = -that
        const int k = (int)((__log2f(a) + 39.863137f) * 7.2725409f);  // log(a / 1e-12) / log(1.1), within one
        idx = v > 0.0f ? mid + 2 + k : mid - 1 - k;
    } else {
        idx = v < 0.0f ? mid : mid + 1;
    }
    idx = min(max(idx, 0), n - 1);
    for (int step = 0; step < 4; ++step) {
        const float above = flim[idx], below = flim[idx > 0 ? idx - 1 : 0];
        if (above <= v) {
            if (idx == n - 1) return idx;
            ++idx;
        } else if (idx > 0 && below > v) {
            --idx;
        } else {
            return idx;
        }
    }
    int lo = 0, hi = n;  // another table than the one the estimate is made for
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (flim[m] > v)
            hi = m;
        else
            lo = m + 1;
    }
    return min(lo, n - 1);
}

struct Acc {
    double sum = 0.0, sq = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    int num = 0, bad = 0;
};

// One element per lane; called by whole wavefronts (`live` masks the lanes that hold an element).
__device__ __forceinline__ void take(Acc& acc, unsigned* hist, const float* flim, int n, int mid, float v, bool live) {
    const bool fin = live && (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
    int b = 0;
    if (fin) {
        const double d = (double)v;
        acc.sum += d;
        acc.sq = fma(d, d, acc.sq);
        acc.mn = fminf(acc.mn, v);
        acc.mx = fmaxf(acc.mx, v);
        ++acc.num;
        b = bucket_of(flim, n, mid, v);
    } else if (live) {
        ++acc.bad;
    }
    const unsigned long long todo = __ballot(fin);
    if (todo == 0) return;
    const int leader = __ffsll((long long)todo) - 1;
    const int lb = __shfl(b, leader);
    const unsigned long long same = __ballot(fin && b == lb);
    if (same == todo) {  // one bucket for the whole wavefront: one add of the lane count
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
    } else if (fin) {
        atomicAdd(&hist[b], 1u);
    }
}

// Fixed-order reduction of one Partial per thread to thread 0 (shuffle tree inside a wavefront, then the wavefronts in
// order).
__device__ __forceinline__ Partial merged(Partial p, const Partial& q) {
    p.mn = fmin(p.mn, q.mn);
    p.mx = fmax(p.mx, q.mx);
    p.sum += q.sum;
    p.sq += q.sq;
    p.num += q.num;
    p.bad += q.bad;
    return p;
}
__device__ __forceinline__ Partial wave_down(Partial p, int d) {  // (for wave_reduce)
    return Partial{__shfl_down(p.mn, d), __shfl_down(p.mx, d), __shfl_down(p.sum, d),
                   __shfl_down(p.sq, d), __shfl_down(p.num, d), __shfl_down(p.bad, d)};
}
__device__ __forceinline__ Partial block_reduce(Partial p, Partial* wred) {
    p = wave_reduce(p, [](Partial a, Partial b) { return merged(a, b); });
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES; ++w) p = merged(p, wred[w]);
    }
    return p;
}

__global__ __launch_bounds__(THREADS) void summary_slice_kernel(const float* __restrict__ base,
                                                                const int64_t* __restrict__ table, int n_segs,
                                                                const double* __restrict__ limits, int n_limits,
                                                                const int64_t* __restrict__ prefix, int64_t ws_slices,
                                                                unsigned long long* __restrict__ buckets,
                                                                Partial* __restrict__ parts) {
    __shared__ float flim[MAXL];
    __shared__ unsigned hist[MAXL];
    __shared__ Partial wred[WAVES];
    if (prefix[n_segs] != ws_slices) return;  // reported by summary_final_kernel
    const int tid = threadIdx.x;
    const int64_t slice = blockIdx.x;
    int lo = 0, hi = n_segs;  // the first entry of prefix[0..n_segs] above `slice`; prefix[n_segs] is
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (prefix[m] > slice)
            hi = m;
        else
            lo = m + 1;
    }
    const int seg = lo - 1;  // prefix[0] = 0 <= slice; empty segments share their successor's prefix and are skipped
    const int64_t first = (slice - prefix[seg]) * SLICE;
    const int n = (int)min(SLICE, table[2 * seg + 1] - first);
    const float* p = base + table[2 * seg] + first;

    for (int i = tid; i < n_limits; i += THREADS) {
        const double l = limits[i];
        float f = (float)l;
        if ((double)f < l) f = nextafterf(f, INFINITY);
        flim[i] = f;
        hist[i] = 0u;
    }
    __syncthreads();

    const int mid = n_limits / 2;
    int head = (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3);  // elements before the first 16-byte boundary
    if (head > n) head = n;
    const int nvec = (n - head) >> 2;
    const int rest = n - 4 * nvec;  // head + tail < 7 elements
    const float4* pv = reinterpret_cast<const float4*>(p + head);
    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    Acc acc;
    for (int i0 = 0; i0 < nvec; i0 += 2 * THREADS) {  // trip count uniform over the block: take() is a wavefront call
        const int i = i0 + tid, j = i + THREADS;
        const bool li = i < nvec, lj = j < nvec;
        const float4 q = li ? pv[i] : none;
        const float4 r = lj ? pv[j] : none;
        take(acc, hist, flim, n_limits, mid, q.x, li);
        take(acc, hist, flim, n_limits, mid, q.y, li);
        take(acc, hist, flim, n_limits, mid, q.z, li);
        take(acc, hist, flim, n_limits, mid, q.w, li);
        take(acc, hist, flim, n_limits, mid, r.x, lj);
        take(acc, hist, flim, n_limits, mid, r.y, lj);
        take(acc, hist, flim, n_limits, mid, r.z, lj);
        take(acc, hist, flim, n_limits, mid, r.w, lj);
    }
    if (tid < 64) {  // the unaligned ends: one wavefront
        const bool live = tid < rest;
        const int e = tid < head ? tid : 4 * nvec + tid;
        take(acc, hist, flim, n_limits, mid, live ? p[e] : 0.f, live);
    }
    __syncthreads();
    unsigned long long* out = buckets + (int64_t)seg * n_limits;
    for (int i = tid; i < n_limits; i += THREADS) {
        const unsigned c = hist[i];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
    Partial mine;
    mine.mn = acc.num ? (double)acc.mn : DBL_MAX;
    mine.mx = acc.num ? (double)acc.mx : -DBL_MAX;
    mine.sum = acc.sum;
    mine.sq = acc.sq;
    mine.num = acc.num;
    mine.bad = acc.bad;
    const Partial total = block_reduce(mine, wred);
    if (tid == 0) parts[slice] = total;
}

__global__ __launch_bounds__(THREADS) void summary_final_kernel(const int64_t* __restrict__ prefix, int n_segs,
                                                                int64_t ws_slices, const Partial* __restrict__ parts,
                                                                double* __restrict__ stats,
                                                                int64_t* __restrict__ nonfinite) {
    __shared__ Partial wred[WAVES];
    const int seg = blockIdx.x;
    if (prefix[n_segs] != ws_slices) {
        if (threadIdx.x == 0) nonfinite[seg] = -1;
        return;
    }
    Partial p = {DBL_MAX, -DBL_MAX, 0.0, 0.0, 0, 0};
    for (int64_t s = prefix[seg] + threadIdx.x; s < prefix[seg + 1]; s += THREADS) p = merged(p, parts[s]);
    p = block_reduce(p, wred);
    if (threadIdx.x == 0) {
        double* o = stats + 5 * (int64_t)seg;
        o[0] = p.mn;
        o[1] = p.mx;
        o[2] = (double)p.num;
        o[3] = p.sum;
        o[4] = p.sq;
        nonfinite[seg] = p.bad;
    }
}

}  // namespace

extern "C" int hypel_tensor_summary_f32(const float* base, const int64_t* table, int32_t n_segs, const double* limits,
                                        int32_t n_limits, double* stats, int64_t* nonfinite, int64_t* buckets, double* ws,
                                        int32_t ws_slices, hypel_stream_t stream) {
    HYPEL_REQUIRE(base && table && limits && stats && nonfinite && buckets && ws, "hypel_tensor_summary_f32");
    HYPEL_REQUIRE(n_segs > 0 && ws_slices >= 0 && n_limits >= 1 && n_limits <= HYPEL_SUMMARY_MAX_LIMITS,
                  "hypel_tensor_summary_f32");
    static_assert(sizeof(Partial) == 6 * sizeof(double), "HYPEL_SUMMARY_WS_DOUBLES");
    int64_t* prefix = reinterpret_cast<int64_t*>(ws);
    Partial* parts = reinterpret_cast<Partial*>(ws + (int64_t)n_segs + 1);
    if (hipMemsetAsync(buckets, 0, (size_t)n_segs * n_limits * sizeof(int64_t), ST) != hipSuccess) {
        hypel_set_error("hypel_tensor_summary_f32: clearing the bucket counts failed");
        return -2;
    }
    hipLaunchKernelGGL(summary_plan_kernel, dim3(1), dim3(THREADS), 0, ST, table, n_segs, prefix);
    if (ws_slices > 0)
        hipLaunchKernelGGL(summary_slice_kernel, dim3(ws_slices), dim3(THREADS), 0, ST, base, table, n_segs, limits,
                           n_limits, prefix, (int64_t)ws_slices, reinterpret_cast<unsigned long long*>(buckets), parts);
    hipLaunchKernelGGL(summary_final_kernel, dim3(n_segs), dim3(THREADS), 0, ST, prefix, n_segs, (int64_t)ws_slices,
                       parts, stats, nonfinite);
    HYPEL_CHECK_LAUNCH("hypel_tensor_summary_f32");
    return 0;
}
