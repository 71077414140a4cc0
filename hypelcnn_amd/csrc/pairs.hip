// Pairing of shadowed and lit pixels for the shadow GAN (gan/gan_sampling_methods.py): from "the shadow map is in
// HBM" to "the two point lists hypel_gather_patches_f32 cuts the pairs from".
//   * mask_dilate_l1   : pixels within L1 distance `radius` of a set pixel (scipy.ndimage.binary_dilation with the
//                        default cross element, `radius` iterations) in two launches, whatever the radius
//   * pair_masks       : the shadow-side and lit-side selection masks of the samplers
//   * mask_compact     : (x, y) of every selected pixel in row-major scan order -- count, scan, scatter
//   * points_expand    : numpy.repeat of a point list plus the remainder rows of the target sampler
// All of them stream bytes: lanes run along a row on consecutive addresses, ranks inside a wave come from a ballot
// and a population count, ranks across waves and blocks from prefix sums in a fixed order -- no atomics, so two runs
// write identical bytes.
#include "compact.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int FAR = 0x3fffffff;  // "no set pixel in this row": |dy| + FAR cannot wrap

// running maximum over the block in thread order (reverse: from the last thread down), own value included; every
// thread also receives the block's maximum
__device__ __forceinline__ int block_scan_max(int v, bool reverse, int* wave_max, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = wave_scan(v, [](int a, int o) { return o > a ? o : a; }, reverse);
    if (lane == (reverse ? 0 : 63)) wave_max[wv] = v;
    __syncthreads();
    int before = -FAR, all = -FAR;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        const int m = wave_max[k];
        if (reverse ? k > wv : k < wv) before = m > before ? m : before;
        all = m > all ? m : all;
    }
    __syncthreads();  // wave_max is written again for the caller's next strip
    *total = all;
    return before > v ? before : v;
}

// ------------------------------------------------------------------------------------------------ dilation
// One block per row, the row in strips of 256 consecutive pixels, lane t of a strip on pixel x0 + t in both sweeps.
// Sweep 0 walks the strips left to right and stores the distance to the nearest set pixel at or left of x: that
// pixel's column is a running maximum of "my column if I am set", handed from strip to strip.  Sweep 1 walks them
// right to left with the running maximum of the negated column -- the nearest set pixel at or right of x -- and keeps
// the smaller distance.  Every lane reads back only what it stored itself.
__global__ void __launch_bounds__(THREADS) row_distance_kernel(const uint8_t* __restrict__ map, int w,
                                                               int32_t* __restrict__ dist) {
    __shared__ int wave_max[WAVES];
    const uint8_t* row = map + (int64_t)blockIdx.x * w;
    int32_t* drow = dist + (int64_t)blockIdx.x * w;
    const int strips = (w + THREADS - 1) / THREADS;
    for (int sweep = 0; sweep < 2; ++sweep) {
        int carry = -FAR;
        for (int s = 0; s < strips; ++s) {
            const int x = (sweep ? strips - 1 - s : s) * THREADS + (int)threadIdx.x;
            const bool in = x < w;
            const int v = in && row[x] != 0 ? (sweep ? -x : x) : -FAR;
            int total;
            int last = block_scan_max(v, sweep != 0, wave_max, &total);
            last = carry > last ? carry : last;
            if (in) {
                const int d = last == -FAR ? FAR : (sweep ? -last - x : x - last);
                if (sweep == 0 || d < drow[x]) drow[x] = d;
            }
            carry = total > carry ? total : carry;
        }
    }
}

// out[y][x] = 1 where some row y + dy, |dy| <= radius, has a set pixel within radius - |dy| of column x.  Lanes run
// along x, so every read of `dist` is a contiguous row segment.
__global__ void __launch_bounds__(THREADS) column_reach_kernel(const int32_t* __restrict__ dist, int64_t h, int64_t w,
                                                               int32_t radius, uint8_t* __restrict__ out) {
    const int64_t x = (int64_t)blockIdx.y * THREADS + threadIdx.x;
    const int64_t y = blockIdx.x;
    if (x >= w) return;
    const int64_t y0 = y - radius < 0 ? 0 : y - radius, y1 = y + radius >= h ? h - 1 : y + radius;
    bool hit = false;
    for (int64_t yy = y0; yy <= y1; ++yy) {
        const int dy = (int)(yy > y ? yy - y : y - yy);
        hit |= dist[yy * w + x] + dy <= radius;
    }
    out[y * w + x] = hit ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ selection masks
__global__ void __launch_bounds__(THREADS) pair_masks_kernel(const uint8_t* __restrict__ map,
                                                             const uint8_t* __restrict__ reach,
                                                             const uint8_t* __restrict__ margin, int64_t n,
                                                             uint8_t* __restrict__ shadow, uint8_t* __restrict__ lit) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const bool sh = map[i] == 1;
        bool li = !sh;
        if (reach) li = li && reach[i] != 0 && margin[i] == 0;
        shadow[i] = sh ? 1 : 0;
        lit[i] = li ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ compaction
// compact.h with "the mask byte is set" as the predicate; a hit writes its (x, y) to its rank's row
struct MaskSet {
    const uint8_t* __restrict__ mask;
    __device__ __forceinline__ bool operator()(int64_t p) const { return mask[p] != 0; }
};

struct PointRow {
    int2* __restrict__ points;
    int64_t capacity;
    uint32_t w;
    __device__ __forceinline__ void operator()(int64_t p, int rank) const {
        const uint32_t y = (uint32_t)p / w;  // h * w < 2^31
        if (rank < capacity) points[rank] = make_int2((int)((uint32_t)p - y * w), (int)y);
    }
    __device__ __forceinline__ void miss(int64_t) const {}
};

// ------------------------------------------------------------------------------------------------ expansion
__global__ void __launch_bounds__(THREADS) points_expand_kernel(const int2* __restrict__ points, int64_t body,
                                                                int32_t repeat, int64_t total,
                                                                int2* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS)
        out[i] = points[i < body ? i / repeat : i - body];
}

}  // namespace

extern "C" int hypel_mask_dilate_l1_u8(const uint8_t* map, int64_t h, int64_t w, int32_t radius, uint8_t* out,
                                       int32_t* ws, hypel_stream_t stream) {
    HYPEL_REQUIRE(map && out && ws && map != out, "hypel_mask_dilate_l1_u8");
    HYPEL_REQUIRE(h > 0 && w > 0 && h < (1ll << 31) && w < 65536ll * THREADS && radius >= 1 && radius < FAR,
                  "hypel_mask_dilate_l1_u8");
    hipLaunchKernelGGL(row_distance_kernel, dim3((unsigned)h), dim3(THREADS), 0, ST, map, (int)w, ws);
    hipLaunchKernelGGL(column_reach_kernel, dim3((unsigned)h, (unsigned)((w + THREADS - 1) / THREADS)), dim3(THREADS),
                       0, ST, ws, h, w, radius, out);
    HYPEL_CHECK_LAUNCH("hypel_mask_dilate_l1_u8");
    return 0;
}

extern "C" int hypel_pair_masks_u8(const uint8_t* map, const uint8_t* reach, const uint8_t* margin, int64_t n,
                                   uint8_t* shadow, uint8_t* lit, hypel_stream_t stream) {
    HYPEL_REQUIRE(map && shadow && lit && shadow != lit && n > 0, "hypel_pair_masks_u8");
    HYPEL_REQUIRE((reach == nullptr) == (margin == nullptr), "hypel_pair_masks_u8");
    hipLaunchKernelGGL(pair_masks_kernel, dim3(hypel_grid_1d(n, THREADS)), dim3(THREADS), 0, ST, map, reach, margin, n,
                       shadow, lit);
    HYPEL_CHECK_LAUNCH("hypel_pair_masks_u8");
    return 0;
}

extern "C" int hypel_mask_compact_points_i32(const uint8_t* mask, int64_t h, int64_t w, int32_t* points,
                                             int64_t capacity, int32_t* count, int32_t* ws, hypel_stream_t stream) {
    HYPEL_REQUIRE(mask && points && count && ws && capacity >= 0, "hypel_mask_compact_points_i32");
    HYPEL_REQUIRE(h > 0 && w > 0 && h < (1ll << 31) && w < (1ll << 31) && h * w < (1ll << 31),
                  "hypel_mask_compact_points_i32");
    compact::launch(MaskSet{mask}, PointRow{(int2*)points, capacity, (uint32_t)w}, h * w, ws, count, ST);
    HYPEL_CHECK_LAUNCH("hypel_mask_compact_points_i32");
    return 0;
}

extern "C" int hypel_points_expand_i32(const int32_t* points, int64_t n, int32_t repeat, int64_t remainder,
                                       int32_t* out, hypel_stream_t stream) {
    HYPEL_REQUIRE(points && out && points != out, "hypel_points_expand_i32");
    HYPEL_REQUIRE(n > 0 && repeat >= 0 && remainder >= 0 && remainder <= n, "hypel_points_expand_i32");
    const int64_t body = n * repeat, total = body + remainder;
    HYPEL_REQUIRE(total > 0, "hypel_points_expand_i32");
    hipLaunchKernelGGL(points_expand_kernel, dim3(hypel_grid_1d(total, THREADS)), dim3(THREADS), 0, ST,
                       (const int2*)points, body, repeat, total, (int2*)out);
    HYPEL_CHECK_LAUNCH("hypel_points_expand_i32");
    return 0;
}
