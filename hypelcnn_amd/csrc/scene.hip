// Scene preparation: from "the raster file's samples are in HBM" to "the padded, normalised float32 scene the patch
// gather reads" (BasicDataSet.__init__, common_nn_ops.py:45-72; AVONDataLoader.load_data's percentile clip; the
// per-band lit/shadow means of calculate_shadow_ratio).
//   * scene_extrema      : per-band min / max of the (optionally clipped, optionally offset) samples
//   * scene_rank_select  : per-band values at two ranks of a uint16 raster, exactly (two-level radix, 8 + 8 bits)
//   * scene_prepare      : symmetric padding + clip + offset + division + float32, one read and one write
//   * scene_masked_sums  : per-band fp64 sums of the prepared scene over the shadow map's two classes
// The source raster is addressed by element strides (sy, sx, sb) so that a transposed view of a file with a band
// window is read in place.  Every kernel that reads the source goes through ONE tile loader: 64 positions along the
// pixel axis with the smaller stride x TB bands, fetched along whichever of the two has the unit (smallest) stride
// -- lanes on consecutive addresses -- into an LDS tile [position][band] with an odd leading dimension; the consumers
// then run with one lane per band (conflict free in both directions).
#include <math.h>

#include <limits>

#include "common.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int TP = 64;       // positions of a tile along the fast pixel axis
constexpr int THREADS = 256;

struct SceneGeom {
    int64_t ext_f, ext_o;  // source extent along the fast / the other pixel axis
    int64_t sf, so, sb;    // element strides of the source along them and along the bands
    int bands;
    int band_fast;  // 1: lanes run over bands when fetching, 0: over the positions of the fast pixel axis
    int y_fast;     // 1: the fast pixel axis is y (rows), 0: x (columns)
};

inline SceneGeom make_geom(int64_t h, int64_t w, int bands, int64_t sy, int64_t sx, int64_t sb) {
    SceneGeom g;
    // an axis of extent 1 never decides the fetch direction, whatever stride it was given (0 for a numpy newaxis)
    const int64_t far = std::numeric_limits<int64_t>::max();
    const int64_t ey = h == 1 ? far : sy, ex = w == 1 ? far : sx, eb = bands == 1 ? far : sb;
    g.y_fast = ey < ex;
    g.ext_f = g.y_fast ? h : w;
    g.ext_o = g.y_fast ? w : h;
    g.sf = g.y_fast ? sy : sx;
    g.so = g.y_fast ? sx : sy;
    g.sb = sb;
    g.bands = bands;
    const int64_t ef = g.y_fast ? ey : ex;
    g.band_fast = eb < ef || (eb == ef && bands >= 16);
    return g;
}

// numpy.pad(mode="symmetric") source index of padded index i - pad: reflection with the edge repeated, period 2n
__device__ __forceinline__ int64_t reflect(int64_t i, int64_t n) {
    int64_t m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

template <typename T>
__device__ __forceinline__ uint32_t to_bits(T v) { return (uint32_t)v; }
template <>
__device__ __forceinline__ uint32_t to_bits<float>(float v) { return __float_as_uint(v); }
template <>
__device__ __forceinline__ uint32_t to_bits<int16_t>(int16_t v) { return (uint32_t)(uint16_t)v; }
template <typename T>
__device__ __forceinline__ T from_bits(uint32_t u) { return (T)u; }
template <>
__device__ __forceinline__ float from_bits<float>(uint32_t u) { return __uint_as_float(u); }

// Tile of padded positions f0 .. f0 + TP - 1 (fast pixel axis) at source line `o_src` (already reflected), bands
// b0 .. b0 + TB - 1.  ext_pad: padded extent along the fast axis.  Entries outside the raster are left untouched.
template <typename T, int TB>
__device__ __forceinline__ void load_tile(const T* __restrict__ src, const SceneGeom& g, int64_t f0, int64_t ext_pad,
                                          int pad, int64_t o_src, int b0, uint32_t (*tile)[TB + 1]) {
    const T* line = src + o_src * g.so;
    if (g.band_fast) {
        const int bb = threadIdx.x % TB;
        if (b0 + bb < g.bands)
            for (int pix = threadIdx.x / TB; pix < TP; pix += THREADS / TB) {
                if (f0 + pix >= ext_pad) break;
                tile[pix][bb] = to_bits<T>(line[reflect(f0 + pix - pad, g.ext_f) * g.sf + (int64_t)(b0 + bb) * g.sb]);
            }
    } else {
        const int pix = threadIdx.x % TP;
        if (f0 + pix < ext_pad) {
            const T* p = line + reflect(f0 + pix - pad, g.ext_f) * g.sf;
            for (int bb = threadIdx.x / TP; bb < TB && b0 + bb < g.bands; bb += THREADS / TP)
                tile[pix][bb] = to_bits<T>(p[(int64_t)(b0 + bb) * g.sb]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ extrema
template <typename T>
__device__ __forceinline__ T hi_identity() { return std::numeric_limits<T>::max(); }
template <>
__device__ __forceinline__ float hi_identity<float>() { return INFINITY; }
template <typename T>
__device__ __forceinline__ T lo_identity() { return std::numeric_limits<T>::lowest(); }
template <>
__device__ __forceinline__ float lo_identity<float>() { return -INFINITY; }

// grid (slices, band tiles of 64): block `s` walks pixel tiles s * tiles_per_block ... and leaves the min / max of
// its share in part[(s * 2 + {0, 1}) * bands + b].  The value reduced is (T)(min(v, clip[b]) - sub[b]) -- the
// arithmetic of the source dtype, wrapping for the integers -- with either step optional.
template <typename T>
__global__ void __launch_bounds__(THREADS) extrema_partial_kernel(const T* __restrict__ src, SceneGeom g,
                                                                  int64_t n_tiles, int64_t tiles_per_block,
                                                                  const T* __restrict__ clip,
                                                                  const T* __restrict__ sub, T* __restrict__ part) {
    constexpr int TB = 64;
    __shared__ uint32_t tile[TP][TB + 1];
    __shared__ uint32_t red[2][THREADS / TB][TB];
    const int b0 = blockIdx.y * TB, bb = threadIdx.x % TB, pg = threadIdx.x / TB;
    const bool live = b0 + bb < g.bands;
    const int64_t tiles_f = (g.ext_f + TP - 1) / TP;
    T mn = hi_identity<T>(), mx = lo_identity<T>();
    T c = T(0), s = T(0);
    if (live && clip) c = clip[b0 + bb];
    if (live && sub) s = sub[b0 + bb];
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
    const int64_t t1 = t0 + tiles_per_block < n_tiles ? t0 + tiles_per_block : n_tiles;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t o = t / tiles_f, f0 = (t - o * tiles_f) * TP;
        load_tile<T, TB>(src, g, f0, g.ext_f, 0, o, b0, tile);
        __syncthreads();
        const int npix = g.ext_f - f0 < TP ? (int)(g.ext_f - f0) : TP;
        if (live)
            for (int pix = pg; pix < npix; pix += THREADS / TB) {
                T v = from_bits<T>(tile[pix][bb]);
                if (clip) v = v < c ? v : c;
                if (sub) v = (T)(v - s);
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
            }
        __syncthreads();
    }
    red[0][pg][bb] = to_bits<T>(mn);
    red[1][pg][bb] = to_bits<T>(mx);
    __syncthreads();
    if (pg == 0 && live) {
        for (int k = 1; k < THREADS / TB; ++k) {
            const T a = from_bits<T>(red[0][k][bb]), b = from_bits<T>(red[1][k][bb]);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        part[((int64_t)blockIdx.x * 2 + 0) * g.bands + b0 + bb] = mn;
        part[((int64_t)blockIdx.x * 2 + 1) * g.bands + b0 + bb] = mx;
    }
}

template <typename T>
__global__ void extrema_final_kernel(const T* __restrict__ part, int slices, int bands, T* __restrict__ out_min,
                                     T* __restrict__ out_max) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bands) return;
    T mn = part[b], mx = part[bands + b];
    for (int s = 1; s < slices; ++s) {
        const T a = part[((int64_t)s * 2) * bands + b], c = part[((int64_t)s * 2 + 1) * bands + b];
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
    out_min[b] = mn;
    out_max[b] = mx;
}

template <typename T>
int launch_extrema(const void* src, const SceneGeom& g, const void* clip, const void* sub, void* out_min, void* out_max,
                   void* ws, int ws_slices, hipStream_t st) {
    const int64_t n_tiles = g.ext_o * ((g.ext_f + TP - 1) / TP);
    const int64_t per = (n_tiles + ws_slices - 1) / ws_slices;
    const int slices = (int)((n_tiles + per - 1) / per);  // <= ws_slices, none empty
    const int band_tiles = (g.bands + 63) / 64;
    hipLaunchKernelGGL(extrema_partial_kernel<T>, dim3(slices, band_tiles), dim3(THREADS), 0, st, (const T*)src, g,
                       n_tiles, per, (const T*)clip, (const T*)sub, (T*)ws);
    hipLaunchKernelGGL(extrema_final_kernel<T>, dim3((g.bands + 63) / 64), dim3(64), 0, st, (const T*)ws, slices,
                       g.bands, (T*)out_min, (T*)out_max);
    return 0;
}

// ------------------------------------------------------------------------------------------------ rank select
constexpr int RB = 32;  // bands of a histogram tile: hist[256][RB + 1] + the pixel tile stay under 48 KiB of LDS

// LEVEL 1: bin = high byte of every value.  LEVEL 2: bin = low byte of the values whose high byte is the bucket
// LEVEL 1 selected for rank r = blockIdx.z of that band (sel[(r * bands + b) * 2]).  Each lane owns a band column of
// the LDS histogram; the block's counts reach ghist[z][band][bin] by integer atomics, zero counts skipped.
template <int LEVEL>
__global__ void __launch_bounds__(THREADS) rank_hist_kernel(const uint16_t* __restrict__ src, SceneGeom g,
                                                            int64_t n_tiles, int64_t tiles_per_block,
                                                            const uint32_t* __restrict__ sel,
                                                            uint32_t* __restrict__ ghist) {
    __shared__ uint32_t hist[256][RB + 1];
    __shared__ uint32_t tile[TP][RB + 1];
    const int b0 = blockIdx.y * RB, bb = threadIdx.x % RB, pg = threadIdx.x / RB;
    const bool live = b0 + bb < g.bands;
    for (int e = threadIdx.x; e < 256 * (RB + 1); e += THREADS) (&hist[0][0])[e] = 0;
    uint32_t bucket = 0;
    if (LEVEL == 2 && live) bucket = sel[((int64_t)blockIdx.z * g.bands + b0 + bb) * 2];
    __syncthreads();
    const int64_t tiles_f = (g.ext_f + TP - 1) / TP;
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
    const int64_t t1 = t0 + tiles_per_block < n_tiles ? t0 + tiles_per_block : n_tiles;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t o = t / tiles_f, f0 = (t - o * tiles_f) * TP;
        load_tile<uint16_t, RB>(src, g, f0, g.ext_f, 0, o, b0, tile);
        __syncthreads();
        const int npix = g.ext_f - f0 < TP ? (int)(g.ext_f - f0) : TP;
        if (live)
            for (int pix = pg; pix < npix; pix += THREADS / RB) {
                const uint32_t v = tile[pix][bb];
                if (LEVEL == 1)
                    atomicAdd(&hist[v >> 8][bb], 1u);
                else if ((v >> 8) == bucket)
                    atomicAdd(&hist[v & 255u][bb], 1u);
            }
        __syncthreads();
    }
    const int nb = g.bands - b0 < RB ? g.bands - b0 : RB;
    uint32_t* out = ghist + ((int64_t)blockIdx.z * g.bands + b0) * 256;
    for (int e = threadIdx.x; e < nb * 256; e += THREADS) {
        const uint32_t c = hist[e & 255][e >> 8];
        if (c) atomicAdd(out + e, c);
    }
}

// LEVEL 1: the bucket that holds rank[r] and the rank inside it -> sel.  LEVEL 2: the low byte -> the value.
template <int LEVEL>
__global__ void rank_pick_kernel(const uint32_t* __restrict__ ghist, int bands, int64_t rank_lo, int64_t rank_hi,
                                 uint32_t* __restrict__ sel, uint16_t* __restrict__ out_lo,
                                 uint16_t* __restrict__ out_hi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * bands) return;
    const int r = i / bands, b = i - r * bands;
    const uint32_t* h = ghist + (LEVEL == 1 ? (int64_t)b : (int64_t)i) * 256;
    int64_t want = LEVEL == 1 ? (r ? rank_hi : rank_lo) : (int64_t)sel[(int64_t)i * 2 + 1];
    int bin = 0;
    for (; bin < 255; ++bin) {
        const int64_t c = h[bin];
        if (want < c) break;
        want -= c;
    }
    if (LEVEL == 1) {
        sel[(int64_t)i * 2] = (uint32_t)bin;
        sel[(int64_t)i * 2 + 1] = (uint32_t)want;
    } else {
        (r ? out_hi : out_lo)[b] = (uint16_t)((sel[(int64_t)i * 2] << 8) | (uint32_t)bin);
    }
}

// ------------------------------------------------------------------------------------------------ prepare
// IEEE division, correctly rounded (no reciprocal; the file is compiled without fast-math)
__device__ __forceinline__ float scene_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}

// grid (pixel tiles of the PADDED scene, band tiles of 64): out[(y * wp + x) * bands + b] =
// float32((T)(min(v, clip[b]) - lo[b])) / scale[b] with v the source sample under the symmetric padding.
template <typename T>
__global__ void __launch_bounds__(THREADS) prepare_kernel(const T* __restrict__ src, SceneGeom g, int pad,
                                                          const T* __restrict__ clip, const T* __restrict__ lo,
                                                          const float* __restrict__ scale, float* __restrict__ out) {
    constexpr int TB = 64;
    __shared__ uint32_t tile[TP][TB + 1];
    const int64_t ext_pad = g.ext_f + 2 * (int64_t)pad, oth_pad = g.ext_o + 2 * (int64_t)pad;
    const int64_t tiles_f = (ext_pad + TP - 1) / TP;
    const int64_t t = blockIdx.x;
    const int64_t o = t / tiles_f, f0 = (t - o * tiles_f) * TP;
    const int b0 = blockIdx.y * TB;
    load_tile<T, TB>(src, g, f0, ext_pad, pad, reflect(o - pad, g.ext_o), b0, tile);
    __syncthreads();
    const int npix = ext_pad - f0 < TP ? (int)(ext_pad - f0) : TP;
    const int nb = g.bands - b0 < TB ? g.bands - b0 : TB;
    const int64_t wp = g.y_fast ? oth_pad : ext_pad;
    for (int e = threadIdx.x; e < npix * nb; e += THREADS) {
        const int pix = e / nb, bb = e - pix * nb, b = b0 + bb;
        T v = from_bits<T>(tile[pix][bb]);
        if (clip) {
            const T c = clip[b];
            v = v < c ? v : c;
        }
        if (lo) v = (T)(v - lo[b]);
        float r = (float)v;
        if (scale) r = scene_div(r, scale[b]);
        const int64_t y = g.y_fast ? f0 + pix : o, x = g.y_fast ? o : f0 + pix;
        out[(y * wp + x) * g.bands + b] = r;
    }
}

template <typename T>
int launch_prepare(const void* src, const SceneGeom& g, int pad, const void* clip, const void* lo, const float* scale,
                   float* out, hipStream_t st) {
    const int64_t tiles = (g.ext_o + 2 * (int64_t)pad) * ((g.ext_f + 2 * (int64_t)pad + TP - 1) / TP);
    hipLaunchKernelGGL(prepare_kernel<T>, dim3((unsigned)tiles, (g.bands + 63) / 64), dim3(THREADS), 0, st,
                       (const T*)src, g, pad, (const T*)clip, (const T*)lo, scale, out);
    return 0;
}

// ------------------------------------------------------------------------------------------------ masked sums
// grid (slices, band tiles of 64).  Lane (pg, b) adds the pixels p0 + pg, p0 + pg + 4, ... of its slice in that
// order, the four partial sums of a band are added in pg order, and the slices are added in slice order by
// masked_final_kernel: one fixed order, no floating-point atomics.  part[(s * 2 + k) * (bands + 1) + b], k = 0: pixels
// with map != 0, k = 1: map == 0; column `bands` holds the pixel counts.
__global__ void __launch_bounds__(THREADS) masked_partial_kernel(const float* __restrict__ scene,
                                                                 const uint8_t* __restrict__ map, int64_t n_pix,
                                                                 int64_t pix_per_block, int bands,
                                                                 double* __restrict__ part) {
    constexpr int TB = 64, PG = THREADS / TB;
    __shared__ double red[2][PG][TB];
    __shared__ double cnt[2][PG];
    const int bb = threadIdx.x % TB, pg = threadIdx.x / TB, b = blockIdx.y * TB + bb;
    const bool live = b < bands;
    const int64_t p0 = (int64_t)blockIdx.x * pix_per_block;
    const int64_t p1 = p0 + pix_per_block < n_pix ? p0 + pix_per_block : n_pix;
    double s_on = 0.0, s_off = 0.0;
    int64_t n_on = 0, n_off = 0;
    for (int64_t p = p0 + pg; p < p1; p += PG) {
        const bool on = map[p] != 0;
        n_on += on;
        n_off += !on;
        if (live) {
            const double v = (double)scene[p * bands + b];
            if (on)
                s_on += v;
            else
                s_off += v;
        }
    }
    red[0][pg][bb] = s_on;
    red[1][pg][bb] = s_off;
    if (bb == 0) {
        cnt[0][pg] = (double)n_on;
        cnt[1][pg] = (double)n_off;
    }
    __syncthreads();
    if (pg == 0) {
        double* row = part + (int64_t)blockIdx.x * 2 * (bands + 1);
        if (live) {
            for (int k = 1; k < PG; ++k) {
                s_on += red[0][k][bb];
                s_off += red[1][k][bb];
            }
            row[b] = s_on;
            row[bands + 1 + b] = s_off;
        }
        if (bb == 0 && blockIdx.y == 0) {
            row[bands] = cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3];
            row[2 * bands + 1] = cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3];
        }
    }
}

__global__ void masked_final_kernel(const double* __restrict__ part, int slices, int bands, double* __restrict__ sums,
                                    int64_t* __restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // column of the [2][bands + 1] row
    if (i >= 2 * (bands + 1)) return;
    double acc = 0.0;
    for (int s = 0; s < slices; ++s) acc += part[(int64_t)s * 2 * (bands + 1) + i];
    const int k = i / (bands + 1), b = i - k * (bands + 1);
    if (b == bands)
        counts[k] = (int64_t)acc;
    else
        sums[(int64_t)k * bands + b] = acc;
}

bool geom_ok(int64_t h, int64_t w, int32_t bands, int64_t sy, int64_t sx, int64_t sb) {
    return h > 0 && w > 0 && bands > 0 && sy >= 0 && sx >= 0 && sb >= 0 && h < (1ll << 31) && w < (1ll << 31);
}

}  // namespace

extern "C" int hypel_scene_extrema(const void* src, int32_t dtype, int64_t h, int64_t w, int32_t bands, int64_t sy,
                                   int64_t sx, int64_t sb, const void* clip, const void* sub, void* out_min,
                                   void* out_max, void* ws, int32_t ws_slices, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && out_min && out_max && ws && ws_slices > 0, "hypel_scene_extrema");
    HYPEL_REQUIRE(geom_ok(h, w, bands, sy, sx, sb), "hypel_scene_extrema");
    const SceneGeom g = make_geom(h, w, bands, sy, sx, sb);
    switch (dtype) {
        case HYPEL_DTYPE_F32: launch_extrema<float>(src, g, clip, sub, out_min, out_max, ws, ws_slices, ST); break;
        case HYPEL_DTYPE_U16: launch_extrema<uint16_t>(src, g, clip, sub, out_min, out_max, ws, ws_slices, ST); break;
        case HYPEL_DTYPE_I16: launch_extrema<int16_t>(src, g, clip, sub, out_min, out_max, ws, ws_slices, ST); break;
        case HYPEL_DTYPE_U8: launch_extrema<uint8_t>(src, g, clip, sub, out_min, out_max, ws, ws_slices, ST); break;
        default: hypel_set_error("hypel_scene_extrema: unsupported dtype %d", (int)dtype); return -1;
    }
    HYPEL_CHECK_LAUNCH("hypel_scene_extrema");
    return 0;
}

extern "C" int hypel_scene_rank_select_u16(const uint16_t* src, int64_t h, int64_t w, int32_t bands, int64_t sy,
                                           int64_t sx, int64_t sb, int64_t rank_lo, int64_t rank_hi, uint16_t* out_lo,
                                           uint16_t* out_hi, uint32_t* ws, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && out_lo && out_hi && ws, "hypel_scene_rank_select_u16");
    HYPEL_REQUIRE(geom_ok(h, w, bands, sy, sx, sb) && h * w < (1ll << 32), "hypel_scene_rank_select_u16");
    HYPEL_REQUIRE(0 <= rank_lo && rank_lo <= rank_hi && rank_hi < h * w, "hypel_scene_rank_select_u16");
    const SceneGeom g = make_geom(h, w, bands, sy, sx, sb);
    uint32_t* hist1 = ws;                               // [bands][256]
    uint32_t* hist2 = ws + (int64_t)bands * 256;        // [2][bands][256]
    uint32_t* sel = ws + (int64_t)bands * 768;          // [2][bands]{bucket, rank inside it}
    if (hipMemsetAsync(ws, 0, (size_t)bands * HYPEL_SCENE_RANK_WS_WORDS * sizeof(uint32_t), ST) != hipSuccess) {
        hypel_set_error("hypel_scene_rank_select_u16: clearing the workspace failed");
        return -2;
    }
    const int64_t n_tiles = g.ext_o * ((g.ext_f + TP - 1) / TP);
    const int64_t per = 64;  // 4096 positions x 32 bands per block amortise clearing and flushing its histogram
    const dim3 grid((unsigned)((n_tiles + per - 1) / per), (bands + RB - 1) / RB, 1);
    const dim3 pick((2 * bands + 63) / 64);
    hipLaunchKernelGGL(rank_hist_kernel<1>, grid, dim3(THREADS), 0, ST, src, g, n_tiles, per, sel, hist1);
    hipLaunchKernelGGL(rank_pick_kernel<1>, pick, dim3(64), 0, ST, hist1, bands, rank_lo, rank_hi, sel, out_lo, out_hi);
    hipLaunchKernelGGL(rank_hist_kernel<2>, dim3(grid.x, grid.y, 2), dim3(THREADS), 0, ST, src, g, n_tiles, per, sel,
                       hist2);
    hipLaunchKernelGGL(rank_pick_kernel<2>, pick, dim3(64), 0, ST, hist2, bands, rank_lo, rank_hi, sel, out_lo, out_hi);
    HYPEL_CHECK_LAUNCH("hypel_scene_rank_select_u16");
    return 0;
}

extern "C" int hypel_scene_prepare_f32(const void* src, int32_t dtype, int64_t h, int64_t w, int32_t bands, int64_t sy,
                                       int64_t sx, int64_t sb, int32_t pad, const void* clip, const void* lo,
                                       const float* scale, float* out, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && out && pad >= 0, "hypel_scene_prepare_f32");
    HYPEL_REQUIRE(geom_ok(h, w, bands, sy, sx, sb), "hypel_scene_prepare_f32");
    const SceneGeom g = make_geom(h, w, bands, sy, sx, sb);
    HYPEL_REQUIRE((g.ext_o + 2 * (int64_t)pad) * ((g.ext_f + 2 * (int64_t)pad + TP - 1) / TP) < (1ll << 31),
                  "hypel_scene_prepare_f32");
    switch (dtype) {
        case HYPEL_DTYPE_F32: launch_prepare<float>(src, g, pad, clip, lo, scale, out, ST); break;
        case HYPEL_DTYPE_U16: launch_prepare<uint16_t>(src, g, pad, clip, lo, scale, out, ST); break;
        case HYPEL_DTYPE_I16: launch_prepare<int16_t>(src, g, pad, clip, lo, scale, out, ST); break;
        case HYPEL_DTYPE_U8: launch_prepare<uint8_t>(src, g, pad, clip, lo, scale, out, ST); break;
        default: hypel_set_error("hypel_scene_prepare_f32: unsupported dtype %d", (int)dtype); return -1;
    }
    HYPEL_CHECK_LAUNCH("hypel_scene_prepare_f32");
    return 0;
}

extern "C" int hypel_scene_masked_sums(const float* scene, const uint8_t* map, int64_t hp, int64_t wp, int32_t bands,
                                       double* sums, int64_t* counts, double* ws, int32_t ws_slices,
                                       hypel_stream_t stream) {
    HYPEL_REQUIRE(scene && map && sums && counts && ws && ws_slices > 0, "hypel_scene_masked_sums");
    HYPEL_REQUIRE(hp > 0 && wp > 0 && bands > 0 && hp < (1ll << 31) && wp < (1ll << 31), "hypel_scene_masked_sums");
    const int64_t n_pix = hp * wp;
    const int64_t per = (n_pix + ws_slices - 1) / ws_slices;
    const int slices = (int)((n_pix + per - 1) / per);
    hipLaunchKernelGGL(masked_partial_kernel, dim3(slices, (bands + 63) / 64), dim3(THREADS), 0, ST, scene, map, n_pix,
                       per, bands, ws);
    hipLaunchKernelGGL(masked_final_kernel, dim3((2 * (bands + 1) + 63) / 64), dim3(64), 0, ST, ws, slices, bands, sums,
                       counts);
    HYPEL_CHECK_LAUNCH("hypel_scene_masked_sums");
    return 0;
}
