// Grey-scale morphology on the channels of a resident scene (classic/morphology.py: MorphologicalProfile).
//   * morph_keys             : float32 view -> dense uint32 keys whose unsigned order is the total order of include/hypel.h
//   * morph_erode_dilate     : minimum / maximum over a disk or a square of radius 0 .. HYPEL_MORPH_MAX_RADIUS
//   * morph_reconstruct_sweep: one sweep of the reconstruction by dilation / erosion of a mask from a marker
//   * morph_profile_store    : keys -> float32 into a channel of the symmetric-padded profile stack
// Everything between the first and the last launch is integer min / max on keys: every output is a bit copy of an input,
// no result depends on an evaluation order, there are no tie rules and no floating-point atomics.
//
// An image is [h][w][c]; the operators treat every channel on its own.  The two raster kernels cut a channel into tiles
// of TW x TH pixels; a block takes (tile, channel) jobs with the stride of the grid and holds the tile with its halo in
// LDS.  erode / dilate: the halo is `radius` pixels, the element is one row span per dy (half-width radius for the
// square, floor(sqrt(radius^2 - dy^2)) for the disk), brute force over the span in LDS.  The sweep: the halo is one pixel
// of min(marker, mask) (max for erosion) and stays fixed while the tile is iterated -- Jacobi steps, all reads of a step
// before its writes -- until no pixel of the tile changes: values only rise (fall) and are bounded by the limit of the
// whole image, so the tile's state is the least fixed point above what was loaded, whatever the schedule.  Blocks never
// read what another block of the same launch writes: the caller ping-pongs two buffers.
#include "common.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int THREADS = 256;
constexpr int TW = HYPEL_MORPH_TILE_W, TH = HYPEL_MORPH_TILE_H;
constexpr int PER = TW * TH / THREADS;  // pixels of one thread in a tile
constexpr int MAX_RADIUS = HYPEL_MORPH_MAX_RADIUS;
constexpr int MAX_BLOCKS = HYPEL_MORPH_MAX_BLOCKS;
constexpr int SW = TW + 2, SH = TH + 2;  // a sweep tile with its halo
static_assert(TW * TH % THREADS == 0 && TW == 64, "a tile is a whole number of block-wide strips of whole waves");
// the largest erode / dilate tile with its halo and the span table, and the sweep tile: far below 160 KiB per CU
static_assert(((TW + 2 * MAX_RADIUS) * (TH + 2 * MAX_RADIUS) + 2 * MAX_RADIUS + 1) * 4 <= 64 * 1024, "dynamic LDS");

__device__ __forceinline__ uint32_t key_of(uint32_t u) { return (u >> 31) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t bits_of(uint32_t k) { return (k >> 31) ? (k & 0x7fffffffu) : ~k; }
__device__ __forceinline__ uint32_t pick(uint32_t a, uint32_t b, bool take_max) {
    return take_max ? (a > b ? a : b) : (a < b ? a : b);
}

// ----------------------------------------------------------------------------------------------------------- keys
__global__ void __launch_bounds__(THREADS) keys_kernel(const uint32_t* __restrict__ x, int64_t w, int32_t c, int64_t sy,
                                                       int64_t sx, int64_t total, uint32_t* __restrict__ keys) {
    for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * THREADS) {
        const int64_t pix = e / c, y = pix / w;
        keys[e] = key_of(x[y * sy + (pix - y * w) * sx + (e - pix * c)]);
    }
}

// --------------------------------------------------------------------------------------------------- erode / dilate
// LDS: the tile with its halo, [TH + 2 r][TW + 2 r], then span[2 r + 1] (the half-width of row dy of the element)
__global__ void __launch_bounds__(THREADS) erode_dilate_kernel(const uint32_t* __restrict__ src, int64_t h, int64_t w,
                                                               int32_t c, int32_t r, int32_t shape, int32_t dilate,
                                                               int64_t tiles_x, int64_t jobs, uint32_t* __restrict__ dst) {
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x;
    const int pw = TW + 2 * r, ph = TH + 2 * r;
    uint32_t* tile = lds;
    int* span = (int*)(lds + pw * ph);
    const uint32_t pad = dilate ? 0u : 0xffffffffu;  // the identity of the operation: an offset outside the raster
    for (int i = tid; i <= 2 * r; i += THREADS) {
        int s = r;
        if (shape == HYPEL_MORPH_DISK) {
            const int rest = r * r - (i - r) * (i - r);
            s = 0;
            while ((s + 1) * (s + 1) <= rest) ++s;
        }
        span[i] = s;
    }
    for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const int64_t t = job / c, ty = t / tiles_x;
        const int ch = (int)(job - t * c);
        const int64_t x0 = (t - ty * tiles_x) * TW, y0 = ty * TH;
        __syncthreads();  // the previous tile has been read (first trip: the spans are written)
        for (int i = tid; i < pw * ph; i += THREADS) {
            const int ly = i / pw, lx = i - ly * pw;
            const int64_t y = y0 + ly - r, x = x0 + lx - r;
            tile[i] = (y >= 0 && y < h && x >= 0 && x < w) ? src[(y * w + x) * c + ch] : pad;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = k * THREADS + tid;
            const int ly = i / TW, lx = i % TW;
            const int64_t y = y0 + ly, x = x0 + lx;
            if (y >= h || x >= w) continue;
            uint32_t acc = pad;
            for (int dy = -r; dy <= r; ++dy) {
                const int s = span[dy + r];
                const uint32_t* row = tile + (ly + r + dy) * pw + lx + r;
                for (int dx = -s; dx <= s; ++dx) acc = pick(acc, row[dx], dilate != 0);
            }
            dst[(y * w + x) * c + ch] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ sweep
__global__ void __launch_bounds__(THREADS) sweep_kernel(const uint32_t* __restrict__ marker,
                                                        const uint32_t* __restrict__ mask, int64_t h, int64_t w, int32_t c,
                                                        int32_t dilate, int64_t tiles_x, int64_t jobs,
                                                        uint32_t* __restrict__ out, int32_t* __restrict__ changed) {
    __shared__ uint32_t m[SH * SW];
    const int tid = threadIdx.x;
    const bool up = dilate != 0;                  // by dilation values rise towards the mask, by erosion they fall
    const uint32_t pad = up ? 0u : 0xffffffffu;
    int differs = 0;
    for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const int64_t t = job / c, ty = t / tiles_x;
        const int ch = (int)(job - t * c);
        const int64_t x0 = (t - ty * tiles_x) * TW, y0 = ty * TH;
        __syncthreads();  // the previous tile has been written out
        for (int i = tid; i < SH * SW; i += THREADS) {
            const int ly = i / SW, lx = i - ly * SW;
            const int64_t y = y0 + ly - 1, x = x0 + lx - 1;
            uint32_t v = pad;
            if (y >= 0 && y < h && x >= 0 && x < w) {
                const int64_t at = (y * w + x) * c + ch;
                v = pick(marker[at], mask[at], !up);  // the clamp: min(marker, mask) by dilation
            }
            m[i] = v;
        }
        uint32_t bound[PER];
        int64_t at[PER];  // -1: outside the raster, stays the identity
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = k * THREADS + tid;
            const int64_t y = y0 + i / TW, x = x0 + i % TW;
            at[k] = (y < h && x < w) ? (y * w + x) * c + ch : -1;
            bound[k] = at[k] >= 0 ? mask[at[k]] : pad;
        }
        __syncthreads();
        // a value moves one pixel per step, and no geodesic path inside the tile is longer than its pixel count
        for (int step = 0; step <= TW * TH; ++step) {
            uint32_t next[PER];
            int moved = 0;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = k * THREADS + tid;
                const uint32_t* p = m + (i / TW + 1) * SW + i % TW + 1;
                uint32_t v = p[0];
                if (at[k] >= 0) {
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) v = pick(v, p[dy * SW + dx], up);
                    v = pick(v, bound[k], !up);
                }
                next[k] = v;
                moved |= v != p[0];
            }
            if (!__syncthreads_or(moved)) break;  // (also: every read of this step lies behind it)
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = k * THREADS + tid;
                m[(i / TW + 1) * SW + i % TW + 1] = next[k];
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (at[k] < 0) continue;
            const int i = k * THREADS + tid;
            const uint32_t v = m[(i / TW + 1) * SW + i % TW + 1];
            out[at[k]] = v;
            differs |= v != marker[at[k]];
        }
    }
    if (__syncthreads_or(differs) && tid == 0) atomicOr(changed, 1);
}

// ------------------------------------------------------------------------------------------------------------ store
__device__ __forceinline__ int64_t reflect(int64_t i, int64_t n) { return i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i); }

__global__ void __launch_bounds__(THREADS) store_kernel(const uint32_t* __restrict__ keys, int64_t h, int64_t w, int32_t c,
                                                        int32_t pad, uint32_t* __restrict__ out, int32_t out_c,
                                                        int32_t chan_offset, int32_t chan_step, int64_t total) {
    const int64_t wp = w + 2 * pad;
    for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * THREADS) {
        const int64_t pix = e / c, yp = pix / wp, xp = pix - yp * wp;
        const int b = (int)(e - pix * c);
        const int64_t y = reflect(yp - pad, h), x = reflect(xp - pad, w);
        out[pix * out_c + chan_offset + (int64_t)b * chan_step] = bits_of(keys[(y * w + x) * c + b]);
    }
}

constexpr int64_t MAX_SIDE = (1ll << 31) - 1, MAX_ELEMS = 1ll << 40, MAX_STRIDE = 1ll << 40;

bool image_ok(int64_t h, int64_t w, int32_t c) {
    return h >= 1 && w >= 1 && c >= 1 && h <= MAX_SIDE && w <= MAX_SIDE && h * w <= MAX_ELEMS && c <= MAX_ELEMS / (h * w);
}

bool apart(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + (uintptr_t)a_bytes <= y || y + (uintptr_t)b_bytes <= x;
}

unsigned blocks_for(int64_t jobs) { return (unsigned)(jobs < MAX_BLOCKS ? jobs : MAX_BLOCKS); }

int64_t tiles_across(int64_t w) { return (w + TW - 1) / TW; }
int64_t tiles_of(int64_t h, int64_t w) { return tiles_across(w) * ((h + TH - 1) / TH); }

}  // namespace

extern "C" int hypel_morph_keys_u32(const float* x, int64_t h, int64_t w, int32_t c, int64_t stride_y, int64_t stride_x,
                                    uint32_t* keys, hypel_stream_t stream) {
    HYPEL_REQUIRE(x && keys, "hypel_morph_keys_u32");
    HYPEL_REQUIRE(image_ok(h, w, c), "hypel_morph_keys_u32");
    HYPEL_REQUIRE(stride_y >= c && stride_x >= c && stride_y <= MAX_STRIDE && stride_x <= MAX_STRIDE, "hypel_morph_keys_u32");
    const int64_t total = h * w * c, span = (h - 1) * stride_y + (w - 1) * stride_x + c;
    HYPEL_REQUIRE(apart(x, span * 4, keys, total * 4), "hypel_morph_keys_u32");
    hipLaunchKernelGGL(keys_kernel, dim3(blocks_for((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, ST,
                       (const uint32_t*)x, w, c, stride_y, stride_x, total, keys);
    HYPEL_CHECK_LAUNCH("hypel_morph_keys_u32");
    return 0;
}

extern "C" int hypel_morph_erode_dilate_u32(const uint32_t* src, int64_t h, int64_t w, int32_t c, int32_t radius,
                                            int32_t shape, int32_t op, uint32_t* dst, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && dst, "hypel_morph_erode_dilate_u32");
    HYPEL_REQUIRE(image_ok(h, w, c), "hypel_morph_erode_dilate_u32");
    HYPEL_REQUIRE(radius >= 0 && radius <= MAX_RADIUS, "hypel_morph_erode_dilate_u32");
    HYPEL_REQUIRE(shape == HYPEL_MORPH_DISK || shape == HYPEL_MORPH_SQUARE, "hypel_morph_erode_dilate_u32");
    HYPEL_REQUIRE(op == HYPEL_MORPH_ERODE || op == HYPEL_MORPH_DILATE, "hypel_morph_erode_dilate_u32");
    HYPEL_REQUIRE(apart(src, h * w * c * 4, dst, h * w * c * 4), "hypel_morph_erode_dilate_u32");
    const int64_t jobs = tiles_of(h, w) * c;
    const size_t lds = (size_t)((TW + 2 * radius) * (TH + 2 * radius) + 2 * radius + 1) * sizeof(uint32_t);
    hipLaunchKernelGGL(erode_dilate_kernel, dim3(blocks_for(jobs)), dim3(THREADS), lds, ST, src, h, w, c, radius, shape,
                       (int32_t)(op == HYPEL_MORPH_DILATE), tiles_across(w), jobs, dst);
    HYPEL_CHECK_LAUNCH("hypel_morph_erode_dilate_u32");
    return 0;
}

extern "C" int hypel_morph_reconstruct_sweep_u32(const uint32_t* marker_in, const uint32_t* mask, int64_t h, int64_t w,
                                                 int32_t c, int32_t op, uint32_t* marker_out, int32_t* changed,
                                                 hypel_stream_t stream) {
    HYPEL_REQUIRE(marker_in && mask && marker_out && changed, "hypel_morph_reconstruct_sweep_u32");
    HYPEL_REQUIRE(image_ok(h, w, c), "hypel_morph_reconstruct_sweep_u32");
    HYPEL_REQUIRE(op == HYPEL_MORPH_ERODE || op == HYPEL_MORPH_DILATE, "hypel_morph_reconstruct_sweep_u32");
    const int64_t bytes = h * w * c * 4;
    HYPEL_REQUIRE(apart(marker_in, bytes, marker_out, bytes) && apart(mask, bytes, marker_out, bytes) &&
                      apart(changed, 4, marker_out, bytes) && apart(changed, 4, marker_in, bytes) &&
                      apart(changed, 4, mask, bytes),
                  "hypel_morph_reconstruct_sweep_u32");
    const int64_t jobs = tiles_of(h, w) * c;
    hipLaunchKernelGGL(sweep_kernel, dim3(blocks_for(jobs)), dim3(THREADS), 0, ST, marker_in, mask, h, w, c,
                       (int32_t)(op == HYPEL_MORPH_DILATE), tiles_across(w), jobs, marker_out, changed);
    HYPEL_CHECK_LAUNCH("hypel_morph_reconstruct_sweep_u32");
    return 0;
}

extern "C" int hypel_morph_profile_store_f32(const uint32_t* keys, int64_t h, int64_t w, int32_t c, int32_t pad, float* out,
                                             int32_t out_c, int32_t chan_offset, int32_t chan_step, hypel_stream_t stream) {
    HYPEL_REQUIRE(keys && out, "hypel_morph_profile_store_f32");
    HYPEL_REQUIRE(image_ok(h, w, c), "hypel_morph_profile_store_f32");
    HYPEL_REQUIRE(pad >= 0 && pad <= h && pad <= w, "hypel_morph_profile_store_f32");
    HYPEL_REQUIRE(out_c >= 1 && chan_offset >= 0 && chan_step >= 1 &&
                      chan_offset + ((int64_t)c - 1) * chan_step < out_c,
                  "hypel_morph_profile_store_f32");
    const int64_t padded = (h + 2 * pad) * (w + 2 * pad);
    HYPEL_REQUIRE(padded <= MAX_ELEMS && padded * out_c <= MAX_ELEMS, "hypel_morph_profile_store_f32");
    HYPEL_REQUIRE(apart(keys, h * w * c * 4, out, padded * out_c * 4), "hypel_morph_profile_store_f32");
    const int64_t total = padded * c;
    hipLaunchKernelGGL(store_kernel, dim3(blocks_for((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, ST, keys, h, w,
                       c, pad, (uint32_t*)out, out_c, chan_offset, chan_step, total);
    HYPEL_CHECK_LAUNCH("hypel_morph_profile_store_f32");
    return 0;
}
