// Layer-activation statistics on the device (include/hypel.h, hypel_view_range_f32 / hypel_view_histogram_f32): the
// range and a histogram over a caller's edge table of a rows x cols float32 view with leading dimension ld, taken where
// the forward pass leaves the activations.  Both launches ACCUMULATE into outputs the caller initialised.
//
//   * A view is dealt to wavefronts in spans of SPAN contiguous elements of one row (a view with cols == ld is one long
//     row).  A span is read once: scalar loads up to the first 16-byte boundary, float4 loads, scalar loads for the rest.
//   * view_range_kernel     : min / max / finite / non-finite per lane, a shuffle tree per wavefront, the wavefronts in
//                             order, then per block two integer atomics on the float32 bits (below) and two 64-bit adds.
//   * view_histogram_kernel : the edges are kept in LDS rounded UP to float32, which compares against a float32 element
//                             exactly as the double does (summary.hip); the bin is estimated with one multiply and
//                             corrected against that table, so the table decides.  One LDS histogram per block, integer
//                             atomics -- a wavefront whose lanes all agree on a bin adds its lane count once -- kept over
//                             all of the block's spans; only the non-zero counters are flushed, with 64-bit integer
//                             atomics.
// Integer atomics only: every result is exact and independent of launch geometry and call order.
#include <float.h>
#include <math.h>

#include "common.h"
#include "wave.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SPAN = 1024;        // elements of one wavefront's span: one round of four float4 loads per lane
constexpr int MAX_BLOCKS = 2048;  // 8 per CU; the spans beyond are taken in a grid stride
constexpr int64_t MAX_ELEMENTS = (int64_t)1 << 37;  // 2^31 * 64: a block's uint32 counters see at most 2^26 elements

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// f.take(v, live) for every element of the view, by whole wavefronts (`live` masks the lanes that hold an element)
template <class F>
__device__ __forceinline__ void walk_spans(const float* __restrict__ src, int64_t rows, int64_t ld, int64_t cols, F& f) {
    const int lane = threadIdx.x & 63;
    const int64_t per_row = (cols + SPAN - 1) / SPAN;
    const int64_t spans = rows * per_row;
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t s = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); s < spans; s += stride) {
        int64_t r, c0;
        if (per_row == 1) {
            r = s, c0 = 0;
        } else if (rows == 1) {
            r = 0, c0 = s * SPAN;
        } else {
            r = s / per_row, c0 = (s - r * per_row) * SPAN;
        }
        const float* p = src + r * ld + c0;
        const int n = (int)min((int64_t)SPAN, cols - c0);
        int head = (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3);  // elements before the first 16-byte boundary
        if (head > n) head = n;
        const int nvec = (n - head) >> 2;
        const int rest = n - 4 * nvec;  // head + tail < 7 elements
        const float4* pv = reinterpret_cast<const float4*>(p + head);
        for (int i0 = 0; i0 < nvec; i0 += 256) {  // trip count uniform over the wavefront: take() is a wavefront call
            float4 q[4];
            bool l[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // four loads in flight per lane
                const int i = i0 + 64 * k + lane;
                l[k] = i < nvec;
                q[k] = l[k] ? pv[i] : none;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + 64 * k >= nvec) break;  // (uniform) a short row ends before the fourth load
                f.take(q[k].x, l[k]);
                f.take(q[k].y, l[k]);
                f.take(q[k].z, l[k]);
                f.take(q[k].w, l[k]);
            }
        }
        if (rest) {  // the unaligned ends
            const bool live = lane < rest;
            const int e = lane < head ? lane : 4 * nvec + lane;
            f.take(live ? p[e] : 0.f, live);
        }
    }
}

// ---- range ----------------------------------------------------------------------------------------------------------
struct RangeTake {
    float mn = FLT_MAX, mx = -FLT_MAX;
    int num = 0, bad = 0;
    __device__ __forceinline__ void take(float v, bool live) {
        const bool fin = live && finite_f32(v);
        mn = fin ? fminf(mn, v) : mn;
        mx = fin ? fmaxf(mx, v) : mx;
        num += fin;
        bad += live && !fin;
    }
};

// min / max of a float32 in memory by integer atomics on its bits: among non-negative floats the signed integer order is
// the float order, among negative ones the unsigned order is the reverse, and a negative float is above every
// non-negative one as an unsigned integer.  v + 0.0f turns -0.0 into +0.0 (the two compare equal).
__device__ __forceinline__ void atomic_min_f32(float* addr, float v) {
    v += 0.0f;
    if (v >= 0.0f)
        atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else
        atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
    v += 0.0f;
    if (v >= 0.0f)
        atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
    else
        atomicMin(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}

__global__ __launch_bounds__(THREADS) void view_range_kernel(const float* __restrict__ src, int64_t rows, int64_t ld,
                                                             int64_t cols, float* __restrict__ range,
                                                             unsigned long long* __restrict__ count) {
    __shared__ float wmn[WAVES], wmx[WAVES];
    __shared__ int64_t wnum[WAVES], wbad[WAVES];
    RangeTake f;
    walk_spans(src, rows, ld, cols, f);
    float mn = wave_reduce(f.mn, [](float a, float b) { return fminf(a, b); });
    float mx = wave_reduce(f.mx, [](float a, float b) { return fmaxf(a, b); });
    const int64_t num = wave_sum((int64_t)f.num), bad = wave_sum((int64_t)f.bad);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        wmn[w] = mn, wmx[w] = mx, wnum[w] = num, wbad[w] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t n = 0, b = 0;
        for (int w = 0; w < WAVES; ++w) {
            mn = fminf(mn, wmn[w]);
            mx = fmaxf(mx, wmx[w]);
            n += wnum[w];
            b += wbad[w];
        }
        if (n) {
            // range[0] only falls and range[1] only rises: a block that cannot move what it reads there (however stale)
            // cannot move the final value either, and leaves the address to the blocks that can
            const float seen_mn = __hip_atomic_load(&range[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float seen_mx = __hip_atomic_load(&range[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (mn < seen_mn) atomic_min_f32(&range[0], mn);
            if (mx > seen_mx) atomic_max_f32(&range[1], mx);
            atomicAdd(&count[0], (unsigned long long)n);
        }
        if (b) atomicAdd(&count[1], (unsigned long long)b);
    }
}

// ---- histogram ------------------------------------------------------------------------------------------------------
// fe[k] = edges[k] rounded up to float32, k < n: the bin of a v in range is the last k with fe[k] <= v
struct HistTake {
    const float* fe;
    unsigned* hist;
    int n;
    float lo, hi, scale;  // fe[0], edges[n] rounded DOWN to float32, n / (edges[n] - edges[0])
    int outside = 0;

    __device__ __forceinline__ int bin_of(float v) const {
        // the estimate only has to be near: a NaN or an infinity of the product (a range beyond float32) ends at a bound
        int idx = (int)fminf(fmaxf((v - lo) * scale, 0.0f), (float)(n - 1));
        for (int step = 0; step < 4; ++step) {
            if (idx < n - 1 && fe[idx + 1] <= v)
                ++idx;
            else if (fe[idx] > v && idx > 0)
                --idx;
            else
                return idx;
        }
        int a = 0, b = n;  // a table that is far from uniform: the first entry above v, minus one
        while (a < b) {
            const int m = (a + b) >> 1;
            if (fe[m] > v)
                b = m;
            else
                a = m + 1;
        }
        return max(a - 1, 0);
    }

    __device__ __forceinline__ void take(float v, bool live) {
        const bool fin = live && finite_f32(v);
        const bool in = fin && v >= lo && v <= hi;
        outside += fin && !in;
        int b = 0;
        if (in) b = bin_of(v);
        const unsigned long long todo = __ballot(in);
        if (todo == 0) return;
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(b, leader);
        const unsigned long long same = __ballot(in && b == lb);
        if (same == todo) {  // one bin for the whole wavefront: one add of the lane count
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
        } else if (in) {
            atomicAdd(&hist[b], 1u);
        }
    }
};

__global__ __launch_bounds__(THREADS) void view_histogram_kernel(const float* __restrict__ src, int64_t rows, int64_t ld,
                                                                 int64_t cols, const double* __restrict__ edges,
                                                                 int n_bins, unsigned long long* __restrict__ counts,
                                                                 unsigned long long* __restrict__ outside) {
    extern __shared__ unsigned lds[];  // float fe[n_bins], unsigned hist[n_bins]
    __shared__ int64_t wout[WAVES];
    float* fe = reinterpret_cast<float*>(lds);
    unsigned* hist = lds + n_bins;
    const int tid = threadIdx.x;
    for (int i = tid; i < n_bins; i += THREADS) {
        const double l = edges[i];
        float f = (float)l;
        if ((double)f < l) f = nextafterf(f, INFINITY);
        fe[i] = f;
        hist[i] = 0u;
    }
    const double first = edges[0], last = edges[n_bins];
    float hi = (float)last;
    if ((double)hi > last) hi = nextafterf(hi, -INFINITY);
    __syncthreads();
    HistTake f{fe, hist, n_bins, fe[0], hi, (float)((double)n_bins / (last - first))};
    walk_spans(src, rows, ld, cols, f);
    const int64_t out = wave_sum((int64_t)f.outside);
    if ((tid & 63) == 0) wout[tid >> 6] = out;
    __syncthreads();
    for (int i = tid; i < n_bins; i += THREADS) {
        const unsigned c = hist[i];
        if (c) atomicAdd(&counts[i], (unsigned long long)c);
    }
    if (tid == 0) {
        int64_t o = 0;
        for (int w = 0; w < WAVES; ++w) o += wout[w];
        if (o) atomicAdd(outside, (unsigned long long)o);
    }
}

int grid_of(int64_t rows, int64_t cols) {
    const int64_t spans = rows * ((cols + SPAN - 1) / SPAN);
    return (int)min((spans + WAVES - 1) / WAVES, (int64_t)MAX_BLOCKS);
}

}  // namespace

// a view whose rows follow each other without a gap is one long row: float4 loads over all of it
#define HYPEL_VIEW_ARGS(name)                                                                                 \
    HYPEL_REQUIRE(rows >= 0 && cols >= 1 && ld >= cols, name);                                                \
    HYPEL_REQUIRE(rows == 0 || (rows <= (MAX_ELEMENTS - 1) / cols && ld <= ((int64_t)1 << 62) / rows), name); \
    if (rows == 0) return 0;                                                                                  \
    int64_t vrows = rows, vcols = cols;                                                                       \
    if (ld == cols) vcols = rows * cols, vrows = 1

extern "C" int hypel_view_range_f32(const float* src, int64_t rows, int64_t ld, int32_t cols, float* range,
                                    int64_t* count, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && range && count, "hypel_view_range_f32");
    HYPEL_VIEW_ARGS("hypel_view_range_f32");
    hipLaunchKernelGGL(view_range_kernel, dim3(grid_of(vrows, vcols)), dim3(THREADS), 0, ST, src, vrows, ld, vcols, range,
                       reinterpret_cast<unsigned long long*>(count));
    HYPEL_CHECK_LAUNCH("hypel_view_range_f32");
    return 0;
}

extern "C" int hypel_view_histogram_f32(const float* src, int64_t rows, int64_t ld, int32_t cols, const double* edges,
                                        int32_t n_bins, int64_t* counts, int64_t* outside, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && edges && counts && outside, "hypel_view_histogram_f32");
    HYPEL_REQUIRE(n_bins >= 1 && n_bins <= HYPEL_ACT_MAX_BINS, "hypel_view_histogram_f32");
    HYPEL_VIEW_ARGS("hypel_view_histogram_f32");
    hipLaunchKernelGGL(view_histogram_kernel, dim3(grid_of(vrows, vcols)), dim3(THREADS),
                       2 * (size_t)n_bins * sizeof(unsigned), ST, src, vrows, ld, vcols, edges, (int)n_bins,
                       reinterpret_cast<unsigned long long*>(counts), reinterpret_cast<unsigned long long*>(outside));
    HYPEL_CHECK_LAUNCH("hypel_view_histogram_f32");
    return 0;
}
