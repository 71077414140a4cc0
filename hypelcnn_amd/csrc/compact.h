// Stream compaction over the pixels of a flattened image -- count, scan, rank -- behind
// hypel_mask_compact_points_i32 (pairs.hip) and hypel_components_compact_i32 (components.hip).
// A tile is HYPEL_COMPACT_TILE consecutive pixels, one per block; wave k of the block owns the k-th quarter and reads
// it in ITEMS strips of 64 consecutive pixels, so rank order is (tile, wave, strip, lane).  Ranks inside a strip come
// from a ballot and a population count, across strips, waves and tiles from sums in that fixed order -- no atomics, so
// two runs write identical bytes.  What is selected and what is written for it are functors passed by value:
//   pred(p)        is pixel p < n selected?
//   emit(p, rank)  pixel p is selected and `rank` selected pixels precede it
//   emit.miss(p)   pixel p < n is not
#pragma once
#include "common.h"
#include "wave.h"

namespace compact {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int ITEMS = HYPEL_COMPACT_TILE / THREADS;  // pixels of one lane in a tile
static_assert(HYPEL_COMPACT_TILE % THREADS == 0, "a compaction tile is a whole number of block-wide strips");

// the ballots of my wavefront's ITEMS strips of tile blockIdx.x, which start at pixel `base`; returns their hits
template <typename Pred>
__device__ __forceinline__ int strip_ballots(Pred pred, int64_t n, int64_t& base, unsigned long long (&bits)[ITEMS]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    base = (int64_t)blockIdx.x * HYPEL_COMPACT_TILE + (int64_t)wv * 64 * ITEMS;
    int count = 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t p = base + j * 64 + lane;
        bits[j] = __ballot(p < n && pred(p));
        count += __popcll(bits[j]);
    }
    return count;
}

template <typename Pred>
__global__ void __launch_bounds__(THREADS) tile_count_kernel(Pred pred, int64_t n, int32_t* __restrict__ tile_count) {
    __shared__ int wave_count[WAVES];
    int64_t base;
    unsigned long long bits[ITEMS];
    const int count = strip_ballots(pred, n, base, bits);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int before, all;
        waves_before<WAVES>(wave_count, before, all);
        tile_count[blockIdx.x] = all;
    }
}

// one block: tile_count[0 .. tiles) becomes its exclusive prefix sum in place, *total the sum
static __global__ void __launch_bounds__(THREADS) tile_scan_kernel(int32_t* __restrict__ tile_count, int64_t tiles,
                                                                   int32_t* __restrict__ total) {
    __shared__ int wave_total[WAVES];
    int carry = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += THREADS) {
        const int64_t t = t0 + threadIdx.x;
        const int own = t < tiles ? tile_count[t] : 0;
        const int v = wave_scan(own, WaveAdd());
        if ((threadIdx.x & 63) == 63) wave_total[threadIdx.x >> 6] = v;
        __syncthreads();
        int before, all;
        waves_before<WAVES>(wave_total, before, all);
        __syncthreads();  // wave_total is written again for the next THREADS tiles
        if (t < tiles) tile_count[t] = carry + before + v - own;
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <typename Pred, typename Emit>
__global__ void __launch_bounds__(THREADS) tile_rank_kernel(Pred pred, Emit emit, int64_t n,
                                                            const int32_t* __restrict__ tile_offset) {
    __shared__ int wave_count[WAVES];
    const int lane = threadIdx.x & 63;
    int64_t base;
    unsigned long long bits[ITEMS];
    const int count = strip_ballots(pred, n, base, bits);
    if (lane == 0) wave_count[threadIdx.x >> 6] = count;
    __syncthreads();
    int before, all;
    waves_before<WAVES>(wave_count, before, all);
    int at = tile_offset[blockIdx.x] + before;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t p = base + j * 64 + lane;
        if ((bits[j] >> lane) & 1ull)
            emit(p, at + wave_rank(bits[j]));
        else if (p < n)
            emit.miss(p);
        at += __popcll(bits[j]);
    }
}

// the three launches; the caller checks them (HYPEL_CHECK_LAUNCH)
template <typename Pred, typename Emit>
void launch(Pred pred, Emit emit, int64_t n, int32_t* tile_ws, int32_t* total, hipStream_t st) {
    const int64_t tiles = (n + HYPEL_COMPACT_TILE - 1) / HYPEL_COMPACT_TILE;
    hipLaunchKernelGGL(tile_count_kernel<Pred>, dim3((unsigned)tiles), dim3(THREADS), 0, st, pred, n, tile_ws);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(THREADS), 0, st, tile_ws, tiles, total);
    hipLaunchKernelGGL((tile_rank_kernel<Pred, Emit>), dim3((unsigned)tiles), dim3(THREADS), 0, st, pred, emit, n,
                       (const int32_t*)tile_ws);
}

}  // namespace compact
