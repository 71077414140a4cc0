// Where one raster lies inside another (utilities/lidar_matcher.py: cv2.matchTemplate TM_CCORR_NORMED + minMaxLoc on
// rasters that cv2.resize INTER_AREA enlarged by integer factors, i.e. replicated).
//   * match_ccorr          : num = sum T' * I' over every window, float32 on the fp32 matrix cores
//   * match_window_energy  : sum of I'^2 over every window, double, two separable passes
//   * match_best           : R = num / sqrt(E_I * E_T) as float32, its maximum and the first index that has it
//   * match_render         : the replicated raster as uint8 grey levels (the reference's figure)
// The enlarged rasters are never materialised: every kernel divides its coordinates by the scale when it loads.
//
// The numerator as a matrix product: for an output tile of 16 rows at (Y0, X0) and template column j,
//   num[Y][X] += sum_m A_j[Y][m] * B_j[m][X],   A_j[Y][m] = T'(m - Y, j)   (zero outside 0 <= m - Y < HT)
//                                               B_j[m][X] = I'(Y0 + m, X0 + X + j)
// A_j is a Toeplitz band of one template column, B_j a window of an image slab shifted by j: both are read from LDS
// slabs that are staged once per (column chunk, row chunk) and shared by the block's two waves; a wave owns 16 x 64
// outputs, four 16x16x4 MFMA tiles that share the A fragment.  m runs over 15 + HT rows, so 15 / (15 + HT) of the MFMA
// work multiplies zeros.  The next chunk's samples are fetched into registers while the current one is multiplied.
#include "common.h"
#include "wave.h"

#define ST ((hipStream_t)stream)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;  // of every kernel but the numerator's
constexpr int WAVES = THREADS / 64;

constexpr int TILE = HYPEL_MATCH_TILE;      // output rows of a block, = M of the MFMA
constexpr int CM = HYPEL_MATCH_ROW_CHUNK;   // image rows of a slab
constexpr int CJ = HYPEL_MATCH_COL_CHUNK;   // template columns of a slab
constexpr int BX = HYPEL_MATCH_BLOCK_COLS;  // output columns of a block
constexpr int CC_THREADS = 128;
constexpr int WAVE_COLS = BX / (CC_THREADS / 64);  // output columns of a wave
constexpr int SUBTILES = WAVE_COLS / 16;
constexpr int IMG_PITCH = 176;              // = 48 mod 64: the four K rows of a B fragment fall on disjoint banks
constexpr int TPL_ROWS = CM + TILE - 1;     // template rows a tile touches per row chunk
constexpr int TPL_PITCH = 49;               // odd: the staging writes walk the banks
constexpr int EXT_PER = CM * CJ / CC_THREADS;                         // samples per thread of the slab's last CJ - 1 columns
constexpr int TPL_PER = (TPL_ROWS * CJ + CC_THREADS - 1) / CC_THREADS;  // ... of the template slab
static_assert(TILE == 16 && BX == CC_THREADS && CJ == 32 && CM % 4 == 0, "a thread per slab column, 16x16x4 tiles");
static_assert(IMG_PITCH >= BX + CJ && TPL_PITCH >= TPL_ROWS, "slab geometry");

// one band, enlarged: H x W replicated pixels over a source read through element strides
struct Band {
    const float* p;
    int64_t sy, sx;
    int32_t H, W, s;
};

__device__ __forceinline__ float band_at(const Band& b, int Y, int X) {
    return b.p[(int64_t)(Y / b.s) * b.sy + (int64_t)(X / b.s) * b.sx];
}

// one thread's share of the two slabs of a chunk, on its way from global memory to LDS.  Image slab: CM rows of
// BX + CJ - 1 columns from (Y0 + m0, X0 + j0); the thread holds column tid of every row and column BX + tid % 32 of
// every fourth row.  Template slab: TPL_ROWS rows from m0 - (TILE - 1) of CJ columns from j0; the thread holds column
// tid % 32 of every fourth row.  Outside the rasters: zeros, not whatever lies there -- a band entry of zero must not
// meet a NaN.
struct Staged {
    float main[CM], ext[EXT_PER], tpl[TPL_PER];
};

__device__ __forceinline__ void fetch_chunk(const Band& img, const Band& tpl, int Y0, int X0, int m0, int j0, int tid,
                                            Staged& st) {
    const int sub = tid >> 5, low = tid & 31;
    const int xa = X0 + j0 + tid, xb = X0 + j0 + BX + low;
    const bool va = xa < img.W, vb = low < CJ - 1 && xb < img.W;
    const float* col_a = img.p + (va ? (int64_t)(xa / img.s) * img.sx : 0);
    const float* col_b = img.p + (vb ? (int64_t)(xb / img.s) * img.sx : 0);
    const int ys = Y0 + m0;
    int q = ys / img.s, r = ys - q * img.s;  // (uniform) row ys + mm of the enlarged image is source row q
#pragma unroll
    for (int mm = 0; mm < CM; ++mm) {
        st.main[mm] = (va && ys + mm < img.H) ? col_a[(int64_t)q * img.sy] : 0.0f;
        if (++r == img.s) {
            r = 0;
            ++q;
        }
    }
#pragma unroll
    for (int it = 0; it < EXT_PER; ++it) {
        const int Y = ys + 4 * it + sub;
        st.ext[it] = (vb && Y < img.H) ? col_b[(int64_t)(Y / img.s) * img.sy] : 0.0f;
    }
    const int j = j0 + low;
    const bool vj = j < tpl.W;
    const float* col_t = tpl.p + (vj ? (int64_t)(j / tpl.s) * tpl.sx : 0);
#pragma unroll
    for (int it = 0; it < TPL_PER; ++it) {
        const int t = m0 + 4 * it + sub - (TILE - 1);
        st.tpl[it] = (vj && 4 * it + sub < TPL_ROWS && t >= 0 && t < tpl.H) ? col_t[(int64_t)(t / tpl.s) * tpl.sy] : 0.0f;
    }
}

__device__ __forceinline__ void store_chunk(const Staged& st, int tid, float* img_s, float* tpl_s) {
    const int sub = tid >> 5, low = tid & 31;
#pragma unroll
    for (int mm = 0; mm < CM; ++mm) img_s[mm * IMG_PITCH + tid] = st.main[mm];
#pragma unroll
    for (int it = 0; it < EXT_PER; ++it) img_s[(4 * it + sub) * IMG_PITCH + BX + low] = st.ext[it];
#pragma unroll
    for (int it = 0; it < TPL_PER; ++it)
        if (4 * it + sub < TPL_ROWS) tpl_s[low * TPL_PITCH + 4 * it + sub] = st.tpl[it];
}

// grid (blocks across, tiles down, splits).  A unit of work is one (column chunk, row chunk) pair; split z takes units
// [z * units_per_split, (z + 1) * units_per_split).  out: the surface itself (one split) or this split's partial one.
__global__ void __launch_bounds__(CC_THREADS) ccorr_kernel(Band img, Band tpl, int32_t hout, int32_t wout,
                                                           int32_t n_row_chunks, int32_t n_units,
                                                           int32_t units_per_split, float* __restrict__ out) {
    __shared__ float img_s[CM * IMG_PITCH];
    __shared__ float tpl_s[CJ * TPL_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = lane & 15, k = lane >> 4;  // A: row n of the tile, B: column n of a sub-tile; both K index k
    const int X0 = blockIdx.x * BX, Y0 = blockIdx.y * TILE;
    const int u0 = blockIdx.z * units_per_split;
    const int u1 = min(n_units, u0 + units_per_split);
    const bool active = X0 + wv * WAVE_COLS < wout;  // (wave-uniform)
    f32x4 acc[SUBTILES];
#pragma unroll
    for (int t = 0; t < SUBTILES; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* a_rd = tpl_s + (k - n + TILE - 1);
    const float* b_rd = img_s + k * IMG_PITCH + wv * WAVE_COLS + n;
    Staged st;
    auto fetch = [&](int u) {
        const int jc = u / n_row_chunks, mc = u - jc * n_row_chunks;
        fetch_chunk(img, tpl, Y0, X0, mc * CM, jc * CJ, tid, st);
    };
    if (u0 < u1) fetch(u0);
    for (int u = u0; u < u1; ++u) {
        __syncthreads();  // the previous slabs have been read
        store_chunk(st, tid, img_s, tpl_s);
        __syncthreads();
        if (u + 1 < u1) fetch(u + 1);  // in flight while this chunk is multiplied
        if (!active) continue;
#pragma unroll 2
        for (int jj = 0; jj < CJ; ++jj) {
#pragma unroll
            for (int mm = 0; mm < CM; mm += 4) {
                const float a = a_rd[jj * TPL_PITCH + mm];
#pragma unroll
                for (int t = 0; t < SUBTILES; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_rd[mm * IMG_PITCH + 16 * t + jj], acc[t], 0, 0, 0);
            }
        }
    }
    if (!active) return;
    out += (int64_t)blockIdx.z * hout * wout;
#pragma unroll
    for (int t = 0; t < SUBTILES; ++t) {
        const int X = X0 + wv * WAVE_COLS + 16 * t + n;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int Y = Y0 + 4 * k + r;
            if (Y < hout && X < wout) out[(int64_t)Y * wout + X] = acc[t][r];
        }
    }
}

__global__ void __launch_bounds__(THREADS) add_partials_kernel(const float* __restrict__ ws, int64_t n, int32_t splits,
                                                               float* __restrict__ num) {
    for (int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * THREADS) {
        float sum = ws[p];
        for (int s = 1; s < splits; ++s) sum += ws[(int64_t)s * n + p];
        num[p] = sum;
    }
}

// ------------------------------------------------------------------------------------------------ window energy
// a wavefront per (source row, 64 outputs): rows[r][x] = sum_{j < win_w} I'(r * s, x + j)^2
__global__ void __launch_bounds__(THREADS) row_window_kernel(Band img, int32_t h_src, int32_t win_w, int32_t wout,
                                                             int32_t n_seg, double* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (gw >= (int64_t)h_src * n_seg) return;
    const int r = (int)(gw / n_seg), x0 = (int)(gw - (int64_t)r * n_seg) * 64;
    const float* row = img.p + (int64_t)r * img.sy;
    auto sq = [&](int64_t X) -> double {
        if (X >= img.W) return 0.0;  // (only under lanes whose output is past the surface)
        const double v = (double)row[(X / img.s) * img.sx];
        return v * v;
    };
    double part = 0.0;
    for (int t = lane; t < win_w; t += 64) part += sq((int64_t)x0 + t);
    const double first = wave_reduce_all(part, WaveAdd());  // the same bits in every lane
    // output x0 + lane = the first window + what entered - what left on the way there: two inclusive scans, shifted
    // by one lane
    double lv = wave_scan(sq((int64_t)x0 + lane), WaveAdd());
    double en = wave_scan(sq((int64_t)x0 + win_w + lane), WaveAdd());
    lv = wave_up(lv, 1);
    en = wave_up(en, 1);
    if (lane == 0) lv = en = 0.0;
    // (a sum of squares: what the subtraction leaves below zero over a stretch of zeros is rounding)
    if (x0 + lane < wout) rows[(int64_t)r * wout + x0 + lane] = fmax((first + en) - lv, 0.0);
}

constexpr int YSEG = 32;
// a thread per (column, YSEG outputs): energy[y][x] = sum_{i < win_h} rows[(y + i) / s][x]
__global__ void __launch_bounds__(THREADS) col_window_kernel(const double* __restrict__ rows, int32_t s, int32_t win_h,
                                                             int32_t hout, int32_t wout, double* __restrict__ energy) {
    const int64_t id = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t n_yseg = (hout + YSEG - 1) / YSEG;
    if (id >= n_yseg * wout) return;
    const int x = (int)(id % wout), y0 = (int)(id / wout) * YSEG;
    const double* col = rows + x;
    double sum = 0.0;
#pragma unroll 8
    for (int i = 0; i < win_h; ++i) sum += col[(int64_t)((y0 + i) / s) * wout];
    energy[(int64_t)y0 * wout + x] = sum;
    for (int d = 1; d < YSEG && y0 + d < hout; ++d) {
        sum += col[(int64_t)((y0 + d + win_h - 1) / s) * wout];
        sum -= col[(int64_t)((y0 + d - 1) / s) * wout];
        energy[(int64_t)(y0 + d) * wout + x] = fmax(sum, 0.0);
    }
}

// ------------------------------------------------------------------------------------------------ score and argmax
// float bits -> unsigned with the same order
__device__ __forceinline__ uint32_t sortable(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ void __launch_bounds__(THREADS) score_kernel(const float* __restrict__ num, const double* __restrict__ energy,
                                                        const double* __restrict__ e_t, int64_t n,
                                                        float* __restrict__ score_map, unsigned long long* key) {
    const double et = *e_t;
    unsigned long long best = 0ull;
    for (int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * THREADS) {
        const double d = energy[p] * et;
        const float r = d == 0.0 ? 0.0f : (float)((double)num[p] / sqrt(d));
        if (score_map) score_map[p] = r;
        // larger score first, then the smaller index (n < 2^31)
        const unsigned long long cand = ((unsigned long long)sortable(r) << 32) | (0xffffffffu - (uint32_t)p);
        best = cand > best ? cand : best;
    }
    best = wave_reduce_all(best, [](unsigned long long a, unsigned long long o) { return o > a ? o : a; });
    if ((threadIdx.x & 63) == 0 && best != 0ull) atomicMax(key, best);
}

// result: the key at byte 8 becomes (float32 score, 0, int64 index)
__global__ void decode_best_kernel(unsigned long long* result) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long key = result[1];
    const uint32_t sb = (uint32_t)(key >> 32);
    const uint32_t bits = (sb & 0x80000000u) ? (sb & 0x7fffffffu) : ~sb;
    result[0] = (unsigned long long)bits;  // little endian: the score at byte 0, zero at byte 4
    result[1] = (unsigned long long)(0xffffffffu - (uint32_t)(key & 0xffffffffull));
}

// ------------------------------------------------------------------------------------------------ figure raster
__device__ __forceinline__ float grey_level(float v, float top) {
#pragma clang fp contract(off)
    const float q = v / top;
    return q * 255.0f;
}

__global__ void __launch_bounds__(THREADS) render_kernel(Band img, const float* __restrict__ max,
                                                         uint8_t* __restrict__ out) {
    const float top = *max;
    const int64_t n = (int64_t)img.H * img.W;
    for (int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * THREADS) {
        const int Y = (int)(p / img.W), X = (int)(p - (int64_t)Y * img.W);
        float g = 0.0f;
        if (top > 0.0f) g = grey_level(band_at(img, Y, X), top);
        out[p] = (uint8_t)(g >= 255.0f ? 255 : (g > 0.0f ? (int)g : 0));
    }
}

constexpr int64_t LIMIT = 1ll << 31;

// h, w > 0, strides >= 0, scale >= 1 and the enlarged raster below 2^31 pixels
bool band_ok(int64_t h, int64_t w, int64_t sy, int64_t sx, int32_t scale) {
    return h > 0 && w > 0 && sy >= 0 && sx >= 0 && scale >= 1 && h < LIMIT && w < LIMIT && h * scale < LIMIT &&
           w * scale < LIMIT && (h * scale) * (w * scale) < LIMIT;
}

Band make_band(const float* p, int64_t h, int64_t w, int64_t sy, int64_t sx, int32_t scale) {
    return Band{p, sy, sx, (int32_t)(h * scale), (int32_t)(w * scale), scale};
}

}  // namespace

extern "C" int hypel_match_ccorr_f32(const float* image, int64_t h, int64_t w, int64_t sy, int64_t sx, int32_t scale,
                                     const float* tmpl, int64_t ht, int64_t wt, int64_t tsy, int64_t tsx, int32_t tscale,
                                     float* num, float* ws, int32_t splits, hypel_stream_t stream) {
    HYPEL_REQUIRE(image && tmpl && num && image != num && tmpl != num, "hypel_match_ccorr_f32");
    HYPEL_REQUIRE(band_ok(h, w, sy, sx, scale) && band_ok(ht, wt, tsy, tsx, tscale), "hypel_match_ccorr_f32");
    HYPEL_REQUIRE(ht * tscale <= h * scale && wt * tscale <= w * scale, "hypel_match_ccorr_f32");
    HYPEL_REQUIRE(splits >= 1 && splits <= HYPEL_MATCH_MAX_SPLITS, "hypel_match_ccorr_f32");
    HYPEL_REQUIRE(splits == 1 || (ws && ws != num && ws != image && ws != tmpl), "hypel_match_ccorr_f32");
    const Band img = make_band(image, h, w, sy, sx, scale), tpl = make_band(tmpl, ht, wt, tsy, tsx, tscale);
    const int64_t hout = img.H - tpl.H + 1, wout = img.W - tpl.W + 1;
    HYPEL_REQUIRE(hout * wout * splits < LIMIT, "hypel_match_ccorr_f32");
    const int64_t tiles_y = (hout + TILE - 1) / TILE, blocks_x = (wout + BX - 1) / BX;
    HYPEL_REQUIRE(tiles_y <= 65535, "hypel_match_ccorr_f32");
    const int n_row_chunks = (TILE - 1 + tpl.H + CM - 1) / CM;
    const int64_t n_units = (int64_t)((tpl.W + CJ - 1) / CJ) * n_row_chunks;  // < 2^31: HT * WT is
    const int per_split = (int)((n_units + splits - 1) / splits);
    hipLaunchKernelGGL(ccorr_kernel, dim3((unsigned)blocks_x, (unsigned)tiles_y, (unsigned)splits), dim3(CC_THREADS), 0,
                       ST, img, tpl, (int32_t)hout, (int32_t)wout, n_row_chunks, (int32_t)n_units, per_split,
                       splits == 1 ? num : ws);
    if (splits > 1)
        hipLaunchKernelGGL(add_partials_kernel, dim3(hypel_grid_1d(hout * wout, THREADS)), dim3(THREADS), 0, ST, ws,
                           hout * wout, splits, num);
    HYPEL_CHECK_LAUNCH("hypel_match_ccorr_f32");
    return 0;
}

extern "C" int hypel_match_window_energy_f64(const float* src, int64_t h, int64_t w, int64_t sy, int64_t sx,
                                             int32_t scale, int64_t win_h, int64_t win_w, double* energy, double* ws,
                                             hypel_stream_t stream) {
    HYPEL_REQUIRE(src && energy && ws && energy != ws && (const void*)src != (const void*)energy &&
                      (const void*)src != (const void*)ws,
                  "hypel_match_window_energy_f64");
    HYPEL_REQUIRE(band_ok(h, w, sy, sx, scale), "hypel_match_window_energy_f64");
    HYPEL_REQUIRE(win_h >= 1 && win_w >= 1 && win_h <= h * scale && win_w <= w * scale, "hypel_match_window_energy_f64");
    const Band img = make_band(src, h, w, sy, sx, scale);
    const int64_t hout = img.H - win_h + 1, wout = img.W - win_w + 1;
    const int64_t n_seg = (wout + 63) / 64, waves = h * n_seg, n_yseg = (hout + YSEG - 1) / YSEG;
    HYPEL_REQUIRE((waves + WAVES - 1) / WAVES < LIMIT, "hypel_match_window_energy_f64");
    hipLaunchKernelGGL(row_window_kernel, dim3((unsigned)((waves + WAVES - 1) / WAVES)), dim3(THREADS), 0, ST, img,
                       (int32_t)h, (int32_t)win_w, (int32_t)wout, (int32_t)n_seg, ws);
    hipLaunchKernelGGL(col_window_kernel, dim3((unsigned)((n_yseg * wout + THREADS - 1) / THREADS)), dim3(THREADS), 0, ST,
                       ws, scale, (int32_t)win_h, (int32_t)hout, (int32_t)wout, energy);
    HYPEL_CHECK_LAUNCH("hypel_match_window_energy_f64");
    return 0;
}

extern "C" int hypel_match_best_f32(const float* num, const double* energy, const double* e_t, int64_t hout,
                                    int64_t wout, float* score_map, void* result, hypel_stream_t stream) {
    HYPEL_REQUIRE(num && energy && e_t && result && num != score_map && (const void*)num != result &&
                      (const void*)energy != result && (const void*)e_t != result && (void*)score_map != result,
                  "hypel_match_best_f32");
    HYPEL_REQUIRE(hout > 0 && wout > 0 && hout < LIMIT && wout < LIMIT && hout * wout < LIMIT, "hypel_match_best_f32");
    HYPEL_REQUIRE(((uintptr_t)result & 7) == 0, "hypel_match_best_f32");
    if (hipMemsetAsync(result, 0, 16, ST) != hipSuccess) {
        hypel_set_error("hypel_match_best_f32: clearing the result record failed");
        return -2;
    }
    unsigned long long* rec = (unsigned long long*)result;
    hipLaunchKernelGGL(score_kernel, dim3(hypel_grid_1d(hout * wout, THREADS)), dim3(THREADS), 0, ST, num, energy, e_t,
                       hout * wout, score_map, rec + 1);
    hipLaunchKernelGGL(decode_best_kernel, dim3(1), dim3(64), 0, ST, rec);
    HYPEL_CHECK_LAUNCH("hypel_match_best_f32");
    return 0;
}

extern "C" int hypel_match_render_u8(const float* src, int64_t h, int64_t w, int64_t sy, int64_t sx, int32_t scale,
                                     const float* max, uint8_t* out, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && max && out && (const void*)src != (const void*)out && (const void*)max != (const void*)out,
                  "hypel_match_render_u8");
    HYPEL_REQUIRE(band_ok(h, w, sy, sx, scale), "hypel_match_render_u8");
    const Band img = make_band(src, h, w, sy, sx, scale);
    hipLaunchKernelGGL(render_kernel, dim3(hypel_grid_1d((int64_t)img.H * img.W, THREADS)), dim3(THREADS), 0, ST, img,
                       max, out);
    HYPEL_CHECK_LAUNCH("hypel_match_render_u8");
    return 0;
}
