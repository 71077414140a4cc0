// Band-ratio statistics of the shadow GANs (create_stats / print_stats of gan_common.py, measure_targets_shadow_ratio):
//   * band_ratio         : ratio = num / den * scale per band, the rows whose bands are all finite, and their count
//   * column_rank_select : per column of a float32 matrix, the values at up to 8 ascending ranks over the kept rows,
//                          exactly -- what numpy.percentile sorts for on the host
// The select is a most-significant-byte radix descent over order-preserving uint32 keys: four levels of 8 bits, each one
// histogram pass and one pick.  Level 1 counts the top byte once per column for all ranks; the levels below count, per
// (rank, column), the next byte of the keys that share the prefix picked so far, two ranks to a pass over the matrix:
// 1 + 3 * ceil(n_ranks / 2) reads of it in all.  A block privatises the counts of 32
// columns x a slice of rows in LDS -- lanes run along the bands, so a wavefront reads 128-byte runs of a few rows and
// every lane owns counter columns of its own: however heavy the ties, only the lanes that hold the same columns of
// different rows (eight, or two without float4 loads) can meet on one counter -- and flushes its non-zero counters
// with integer atomics.  (Measured with 90 % of every column at one value: 2 to 4 % slower than without ties at
// 500 000 rows, which is all a wavefront-wide merge of equal counters, as summary.hip has it, could win back.)
// Integer counts only: two calls give identical bits.
#include "common.h"
#include "wave.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int THREADS = 256;
constexpr int CB = 32;             // columns of a histogram tile: hist[256][CB + 1] is 33 KiB of LDS
constexpr int MAX_RANKS = HYPEL_COLUMN_RANK_MAX_RANKS;
constexpr int MAX_SLICE = 4096;    // rows of a block's slice: a 16-bit half of a histogram word cannot overflow
static_assert(MAX_SLICE < 65536, "slice rows");

struct Ranks {
    uint32_t r[MAX_RANKS];
};

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ascending float order == ascending unsigned order of the key (-0.0 sorts right below +0.0)
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// IEEE division, correctly rounded, then the multiplication, each rounded on its own (no reciprocal, no fma)
__device__ __forceinline__ float ratio_of(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}
__device__ __forceinline__ float scaled(float q, float s) {
#pragma clang fp contract(off)
    return q * s;
}

// ------------------------------------------------------------------------------------------------ ratio
// G lanes (a power of two, 1 .. 64) share a row, so a wavefront holds 64 / G rows and walks their bands G at a time:
// G = 64 for the spectra this is made for, smaller for narrow matrices so that their lanes are not idle.
__global__ void __launch_bounds__(THREADS) band_ratio_kernel(const float* __restrict__ num, int64_t ld_num,
                                                             const float* __restrict__ den, int64_t ld_den, int64_t n,
                                                             int bands, int g_shift, const float* __restrict__ scale,
                                                             float* __restrict__ ratio, int64_t ld_ratio,
                                                             uint8_t* __restrict__ row_ok,
                                                             unsigned long long* __restrict__ kept) {
    const int G = 1 << g_shift, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (G - 1), first = lane - sub;  // first lane of this row's group
    const int64_t rows_per_wave = 64 >> g_shift;
    const int64_t rows_per_pass = rows_per_wave * (THREADS / 64) * gridDim.x;
    const unsigned long long group = G == 64 ? ~0ull : ((1ull << G) - 1ull) << first;
    unsigned int mine = 0;  // kept rows this lane reported (group leaders only)
    for (int64_t base = 0; base < n; base += rows_per_pass) {  // trip count uniform over the grid
        const int64_t i = base + ((int64_t)blockIdx.x * (THREADS / 64) + wave) * rows_per_wave + (lane >> g_shift);
        const bool row = i < n;
        bool bad = false;
        if (row) {
            const float* a = num + i * ld_num;
            const float* d = den + i * ld_den;
            float* o = ratio + i * ld_ratio;
            for (int b = sub; b < bands; b += G) {
                float q = ratio_of(a[b], d[b]);
                if (scale) q = scaled(q, scale[b]);
                o[b] = q;
                bad |= !finite_bits(q);
            }
        }
        const unsigned long long any_bad = __ballot(bad);
        if (row && sub == 0) {
            const bool ok = (any_bad & group) == 0ull;
            row_ok[i] = ok ? 1 : 0;
            mine += ok;
        }
    }
    // one integer add per block: adds to one address queue up behind each other, a few thousand of them cost more
    // than the ratios of the validation sample
    __shared__ unsigned int per_wave[THREADS / 64];
    mine = wave_sum(mine);
    if (lane == 0) per_wave[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int all = 0;
        for (int w = 0; w < THREADS / 64; ++w) all += per_wave[w];
        if (all) atomicAdd(kept, (unsigned long long)all);
    }
}

// ------------------------------------------------------------------------------------------------ rank select
// grid (row slices, column tiles of CB, rank pairs).  FIRST: bin = top byte of every kept key, one histogram per column.
// Otherwise: bin = byte `shift / 8` of the kept keys whose bits above it equal the prefix picked for that column
// (sel[(r * bands + b) * 2]) for rank r = 2z or 2z + 1: a key has one bin whichever rank it counts for, so the two
// counts share a word of the LDS histogram, 16 bits each -- a slice is at most MAX_SLICE rows, neither half can carry
// -- and an element costs one LDS atomic for both.
// A lane owns LC neighbouring columns: 4, fetched as one float4, where the matrix allows it (VEC: base and row stride
// multiples of 16 bytes; a lane whose columns straddle the last band falls back to single loads), else 1.  It fetches
// the mask bytes of U rows, then their values (a masked row is never read), then counts: U loads in flight instead
// of two dependent ones per row.
template <bool FIRST, bool VEC>
__global__ void __launch_bounds__(THREADS) column_hist_kernel(const float* __restrict__ x, int64_t ld, int64_t n,
                                                              int bands, const uint8_t* __restrict__ row_ok,
                                                              int64_t rows_per_block, int shift, int n_ranks,
                                                              const uint32_t* __restrict__ sel,
                                                              uint32_t* __restrict__ ghist) {
    constexpr int LC = VEC ? 4 : 1, LANES = CB / LC, ROWS = THREADS / LANES, U = VEC ? 4 : 8;
    __shared__ uint32_t hist[256][CB + 1];
    const int b0 = blockIdx.y * CB, c0 = (threadIdx.x % LANES) * LC, pg = threadIdx.x / LANES;
    const int left = bands - (b0 + c0), ncol = left < 0 ? 0 : left < LC ? left : LC;  // live columns of this lane
    const int rank_a = 2 * blockIdx.z;
    const bool pair = rank_a + 1 < n_ranks;
    for (int e = threadIdx.x; e < 256 * (CB + 1); e += THREADS) (&hist[0][0])[e] = 0;
    uint32_t prefix_a[LC], prefix_b[LC];
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        prefix_a[j] = 0u;
        prefix_b[j] = 0xffffffffu;  // (a prefix has at most 24 bits: all ones matches no key)
        if (!FIRST && j < ncol) {
            prefix_a[j] = sel[((int64_t)rank_a * bands + b0 + c0 + j) * 2];
            if (pair) prefix_b[j] = sel[((int64_t)(rank_a + 1) * bands + b0 + c0 + j) * 2];
        }
    }
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    if (ncol > 0) {
        const float* col = x + b0 + c0;
        for (int64_t i0 = r0 + pg; i0 < r1; i0 += ROWS * U) {
            bool use[U];
            uint32_t k[U][LC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = i0 + u * ROWS;
                use[u] = i < r1 && (!row_ok || row_ok[i] != 0);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < LC; ++j) k[u][j] = 0u;
                if (!use[u]) continue;
                const float* p = col + (i0 + u * ROWS) * ld;
                if (VEC && ncol == LC) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    k[u][0] = key_of(v.x);
                    k[u][LC > 1 ? 1 : 0] = key_of(v.y);
                    k[u][LC > 2 ? 2 : 0] = key_of(v.z);
                    k[u][LC > 3 ? 3 : 0] = key_of(v.w);
                } else {
#pragma unroll
                    for (int j = 0; j < LC; ++j)
                        if (j < ncol) k[u][j] = key_of(p[j]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!use[u]) continue;
#pragma unroll
                for (int j = 0; j < LC; ++j) {
                    if (j >= ncol) break;
                    if (FIRST) {
                        atomicAdd(&hist[k[u][j] >> 24][c0 + j], 1u);
                    } else {
                        const uint32_t top = k[u][j] >> (shift + 8);
                        const uint32_t inc = (top == prefix_a[j] ? 1u : 0u) | (top == prefix_b[j] ? 0x10000u : 0u);
                        if (inc) atomicAdd(&hist[(k[u][j] >> shift) & 255u][c0 + j], inc);
                    }
                }
            }
        }
    }
    __syncthreads();
    const int nb = bands - b0 < CB ? bands - b0 : CB;
    uint32_t* out = ghist + ((int64_t)rank_a * bands + b0) * 256;
    uint32_t* out_b = out + (int64_t)bands * 256;  // rank 2z + 1: its half is zero when there is no such rank
    for (int e = threadIdx.x; e < nb * 256; e += THREADS) {
        const uint32_t c = hist[e & 255][e >> 8];
        if (FIRST) {
            if (c) atomicAdd(out + e, c);
        } else {
            if (c & 0xffffu) atomicAdd(out + e, c & 0xffffu);
            if (c >> 16) atomicAdd(out_b + e, c >> 16);
        }
    }
}

// One wavefront per (rank, column): four bins per lane, a shuffle scan, and the lane whose bins hold the wanted rank
// writes the longer prefix and the rank inside the bin; the last level writes the value.  A per-rank histogram is
// cleared once read, for the next level.
template <bool FIRST>
__global__ void __launch_bounds__(64) column_pick_kernel(uint32_t* __restrict__ ghist, int bands, Ranks ranks,
                                                         uint32_t* __restrict__ sel, float* __restrict__ out) {
    const int i = blockIdx.x, r = i / bands, b = i - r * bands, lane = threadIdx.x;
    uint4* h = reinterpret_cast<uint4*>(ghist + (FIRST ? (int64_t)b : (int64_t)i) * 256);
    const uint4 c = h[lane];
    if (!FIRST) h[lane] = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t want = FIRST ? ranks.r[r] : sel[(int64_t)i * 2 + 1];
    const uint32_t prefix = FIRST ? 0u : sel[(int64_t)i * 2];
    const uint32_t s = c.x + c.y + c.z + c.w;
    const uint32_t incl = wave_scan(s, WaveAdd());
    const uint32_t excl = incl - s;
    const unsigned long long hit = __ballot(want >= excl && want < incl);
    // (no lane only if `kept` was not the number of kept rows: the result is then meaningless, the accesses still safe)
    const int owner = hit ? __ffsll((long long)hit) - 1 : 63;
    if (lane != owner) return;
    uint32_t w = want - excl;
    int bin = 4 * lane;
    if (w >= c.x) {
        w -= c.x;
        ++bin;
        if (w >= c.y) {
            w -= c.y;
            ++bin;
            if (w >= c.z) {
                w -= c.z;
                ++bin;
            }
        }
    }
    const uint32_t longer = (prefix << 8) | (uint32_t)bin;
    sel[(int64_t)i * 2] = longer;
    sel[(int64_t)i * 2 + 1] = w;
    if (out) out[i] = value_of(longer);
}

}  // namespace

extern "C" int hypel_band_ratio_f32(const float* num, int64_t ld_num, const float* den, int64_t ld_den, int64_t n,
                                    int32_t bands, const float* scale, float* ratio, int64_t ld_ratio, uint8_t* row_ok,
                                    int64_t* kept, hypel_stream_t stream) {
    HYPEL_REQUIRE(num && den && ratio && row_ok && kept, "hypel_band_ratio_f32");
    HYPEL_REQUIRE(n >= 1 && n < (1ll << 31) && bands >= 1, "hypel_band_ratio_f32");
    HYPEL_REQUIRE(ld_num >= bands && ld_den >= bands && ld_ratio >= bands, "hypel_band_ratio_f32");
    if (hipMemsetAsync(kept, 0, sizeof(int64_t), ST) != hipSuccess) {
        hypel_set_error("hypel_band_ratio_f32: clearing the count failed");
        return -2;
    }
    int g_shift = 0;
    while (g_shift < 6 && (1 << g_shift) < bands) ++g_shift;
    const int64_t rows_per_block = (int64_t)(THREADS / 64) * (64 >> g_shift);
    const int grid = hypel_grid_1d(n, (int)rows_per_block);
    hipLaunchKernelGGL(band_ratio_kernel, dim3(grid), dim3(THREADS), 0, ST, num, ld_num, den, ld_den, n, (int)bands,
                       g_shift, scale, ratio, ld_ratio, row_ok, reinterpret_cast<unsigned long long*>(kept));
    HYPEL_CHECK_LAUNCH("hypel_band_ratio_f32");
    return 0;
}

extern "C" int hypel_column_rank_select_f32(const float* x, int64_t ld, int64_t n, int32_t bands, const uint8_t* row_ok,
                                            int64_t kept, const int64_t* ranks, int32_t n_ranks, float* out,
                                            uint32_t* ws, hypel_stream_t stream) {
    HYPEL_REQUIRE(x && ranks && out && ws && ((uintptr_t)ws & 15) == 0, "hypel_column_rank_select_f32");
    HYPEL_REQUIRE(n >= 1 && n < (1ll << 31) && bands >= 1 && ld >= bands, "hypel_column_rank_select_f32");
    HYPEL_REQUIRE(bands <= HYPEL_COLUMN_RANK_MAX_BANDS, "hypel_column_rank_select_f32");  // column tiles are grid.y
    HYPEL_REQUIRE(n_ranks >= 1 && n_ranks <= MAX_RANKS, "hypel_column_rank_select_f32");
    HYPEL_REQUIRE(kept >= 1 && kept <= n && (row_ok || kept == n), "hypel_column_rank_select_f32");
    Ranks rk = {};
    for (int r = 0; r < n_ranks; ++r) {
        HYPEL_REQUIRE(ranks[r] >= 0 && ranks[r] < kept, "hypel_column_rank_select_f32");
        rk.r[r] = (uint32_t)ranks[r];
    }
    uint32_t* hist1 = ws;                                          // [bands][256]
    uint32_t* hist_r = ws + (int64_t)bands * 256;                  // [MAX_RANKS][bands][256], reused by levels 2 .. 4
    uint32_t* sel = ws + (int64_t)bands * 256 * (1 + MAX_RANKS);   // [MAX_RANKS][bands]{prefix, rank inside it}
    if (hipMemsetAsync(ws, 0, (size_t)bands * HYPEL_COLUMN_RANK_WS_WORDS * sizeof(uint32_t), ST) != hipSuccess) {
        hypel_set_error("hypel_column_rank_select_f32: clearing the workspace failed");
        return -2;
    }
    // enough blocks to fill the device on the 6 000-row validation sample, slices long enough (<= MAX_SLICE rows) to
    // amortise clearing and flushing a block's histogram on a scene's pairs
    const int col_tiles = (bands + CB - 1) / CB;
    int64_t per = (n * col_tiles + 1023) / 1024;
    per = per < 256 ? 256 : per > MAX_SLICE ? MAX_SLICE : per;
    per = (per + 31) / 32 * 32;
    const unsigned slices = (unsigned)((n + per - 1) / per);
    const dim3 pick((unsigned)(n_ranks * bands));
    const bool vec = (((uintptr_t)x) & 15) == 0 && ld % 4 == 0;
    const dim3 first(slices, col_tiles, 1), rest(slices, col_tiles, (n_ranks + 1) / 2);
    if (vec)
        hipLaunchKernelGGL((column_hist_kernel<true, true>), first, dim3(THREADS), 0, ST, x, ld, n, (int)bands, row_ok,
                           per, 24, (int)n_ranks, sel, hist1);
    else
        hipLaunchKernelGGL((column_hist_kernel<true, false>), first, dim3(THREADS), 0, ST, x, ld, n, (int)bands, row_ok,
                           per, 24, (int)n_ranks, sel, hist1);
    hipLaunchKernelGGL(column_pick_kernel<true>, pick, dim3(64), 0, ST, hist1, (int)bands, rk, sel, (float*)nullptr);
    for (int shift = 16; shift >= 0; shift -= 8) {
        if (vec)
            hipLaunchKernelGGL((column_hist_kernel<false, true>), rest, dim3(THREADS), 0, ST, x, ld, n, (int)bands,
                               row_ok, per, shift, (int)n_ranks, sel, hist_r);
        else
            hipLaunchKernelGGL((column_hist_kernel<false, false>), rest, dim3(THREADS), 0, ST, x, ld, n, (int)bands,
                               row_ok, per, shift, (int)n_ranks, sel, hist_r);
        hipLaunchKernelGGL(column_pick_kernel<false>, pick, dim3(64), 0, ST, hist_r, (int)bands, rk, sel,
                           shift == 0 ? out : (float*)nullptr);
    }
    HYPEL_CHECK_LAUNCH("hypel_column_rank_select_f32");
    return 0;
}
