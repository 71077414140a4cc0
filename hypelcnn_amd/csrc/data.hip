// Data-side kernels of the hot path: everything between "the scene is resident in HBM" and "a batch of
// [N,P,P,C] patches enters the first GEMM", plus the scatter of predictions into the label raster.
//   * gather_patches   : BasicDataSet.get_data_point for a whole batch of targets (common_nn_ops.py:169-185,
//                        InMemoryImporter.py:27-38, GeneratorImporter) -- one launch instead of a Python loop
//   * augment_patches  : the training iterator's map stage (common_nn_ops.py:376-440) fused into the batch
//                        gather: index_select + rot90^k + shadow (per-band ratio, or a pre-computed generator
//                        output) + left/right and up/down flips + per-channel spectral shift, one pass
//   * argmax_scatter   : perform_prediction (common_nn_ops.py:313-327): argmax of the logits written straight
//                        into the uint8 label raster at the target's (x, y)
//   * denorm_scatter   : the GAN scene conversion's ((g * casi_max) + casi_min).astype(dtype)
//                        (gan/gan_infer_image_for_shadow.py:84-85), per pixel row, into the output raster
//   * hsi_to_srgb      : the sRGB rendering of that raster (common/hsi_rgb_converter.py, CIE 1931 2 degree observer,
//                        illuminant E; gan/gan_infer_image_for_shadow.py:97-104)
// The gathers, the augmentation and the scatters are pure HBM streaming: one read and one write of every patch element,
// channel-contiguous so that consecutive lanes touch consecutive addresses (C >= 49 floats per pixel in every
// configuration).  hsi_to_srgb reads a span of each pixel's bands and writes three samples per pixel.
#include "common.h"

#define ST ((hipStream_t)stream)

namespace {

// one block row of 256 lanes walks (sample, pixel) pairs; lanes run over the channels of that pixel
__global__ void gather_patches_kernel(const float* __restrict__ casi, const float* __restrict__ lidar, int64_t wp,
                                      int cc, int cl, const int32_t* __restrict__ points, int64_t n, int p,
                                      float* __restrict__ out) {
    const int c = cc + cl;
    const int npix = p * p;
    const int64_t total = n * npix;
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const int64_t s = item / npix;
        const int pix = (int)(item - s * npix);
        const int py = pix / p, px = pix - py * p;
        const int64_t x0 = points[2 * s], y0 = points[2 * s + 1];
        const int64_t src = (y0 + py) * wp + (x0 + px);
        float* o = out + item * c;
        const float* a = casi + src * cc;
        for (int ch = threadIdx.x; ch < cc; ch += blockDim.x) o[ch] = a[ch];
        if (cl > 0) {
            const float* l = lidar + src * cl;
            for (int ch = threadIdx.x; ch < cl; ch += blockDim.x) o[cc + ch] = l[ch];
        }
    }
}

// GRSS2018: the hyperspectral raster has HALF the resolution of the LiDAR raster the targets are given in
// (loader/GRSS2018DataLoader.py:12-44): patch pixel (py, px) takes its spectrum from
// casi[sy + py/2][sx + px/2] with s = coordinate/2 + nb - nb/2 (both rasters are padded by nb) and its height from
// lidar[y + py][x + px].
__global__ void gather_patches_2x_kernel(const float* __restrict__ casi, const float* __restrict__ lidar,
                                         int64_t casi_wp, int64_t lidar_wp, int cc, int cl, int nb,
                                         const int32_t* __restrict__ points, int64_t n, int p,
                                         float* __restrict__ out) {
    const int c = cc + cl;
    const int npix = p * p;
    const int64_t total = n * npix;
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const int64_t s = item / npix;
        const int pix = (int)(item - s * npix);
        const int py = pix / p, px = pix - py * p;
        const int64_t x0 = points[2 * s], y0 = points[2 * s + 1];
        const int64_t sx = (x0 >> 1) + nb - (nb >> 1), sy = (y0 >> 1) + nb - (nb >> 1);
        const float* a = casi + ((sy + (py >> 1)) * casi_wp + sx + (px >> 1)) * cc;
        float* o = out + item * c;
        for (int ch = threadIdx.x; ch < cc; ch += blockDim.x) o[ch] = a[ch];
        const float* l = lidar + ((y0 + py) * lidar_wp + x0 + px) * cl;
        for (int ch = threadIdx.x; ch < cl; ch += blockDim.x) o[cc + ch] = l[ch];
    }
}

__global__ void augment_patches_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx, int64_t n, int p,
                                       int c, const int32_t* __restrict__ rot_k,
                                       const uint8_t* __restrict__ shadow_pick, const float* __restrict__ shadow_ratio,
                                       const float* __restrict__ shadow_alt, const uint8_t* __restrict__ flip_lr,
                                       const uint8_t* __restrict__ flip_ud, const float* __restrict__ delta,
                                       float* __restrict__ out) {
    const int npix = p * p;
    const int64_t total = n * npix;
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const int64_t s = item / npix;
        const int pix = (int)(item - s * npix);
        int i = pix / p, j = pix - i * p;
        // undo the maps in reverse order of application: up/down flip, left/right flip, then the rotation
        if (flip_ud && flip_ud[s]) i = p - 1 - i;
        if (flip_lr && flip_lr[s]) j = p - 1 - j;
        const int k = rot_k ? rot_k[s] : 0;
        int si = i, sj = j;
        if (k == 1) {  // counter-clockwise quarter turn: out[i][j] = in[j][P-1-i]
            si = j;
            sj = p - 1 - i;
        } else if (k == 2) {
            si = p - 1 - i;
            sj = p - 1 - j;
        } else if (k == 3) {
            si = p - 1 - j;
            sj = i;
        }
        const bool shade = shadow_pick && shadow_pick[s];
        const int64_t src_s = idx ? idx[s] : s;
        // the shadow operators act per pixel spectrum, so they commute with the spatial maps
        const float* src = (shade && shadow_alt) ? shadow_alt + (s * npix + si * p + sj) * c
                                                 : x + (src_s * npix + si * p + sj) * c;
        float* o = out + item * c;
        const float* d = delta ? delta + s * c : nullptr;
        for (int ch = threadIdx.x; ch < c; ch += blockDim.x) {
            float v = src[ch];
            if (shade && shadow_ratio) v = v / shadow_ratio[ch];
            if (d) v = v + d[ch];
            o[ch] = v;
        }
    }
}

__global__ void argmax_scatter_kernel(const float* __restrict__ logits, int64_t ld, int64_t n, int c,
                                      const int32_t* __restrict__ points, uint8_t* __restrict__ raster,
                                      int64_t raster_w) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* z = logits + i * ld;
    int best = 0;
    float bv = z[0];
    for (int j = 1; j < c; ++j)
        if (z[j] > bv) {  // first maximum wins, as tf.argmax
            bv = z[j];
            best = j;
        }
    raster[(int64_t)points[2 * i + 1] * raster_w + points[2 * i]] = (uint8_t)best;
}

// One (normal, shadow) spectrum pair per 64-lane row pass: gather + the regulariser swap of
// perform_shadow_augmentation_random (gan/gan_train_for_shadow.py:171-182).
__global__ void gather_pairs_kernel(const float* __restrict__ normal, const float* __restrict__ shadow,
                                    const int64_t* __restrict__ idx, int64_t n, int bands, const float* __restrict__ ratio,
                                    const float* __restrict__ u1, const float* __restrict__ u2, float rate,
                                    float* __restrict__ out_x, float* __restrict__ out_y) {
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t src = idx[i];
        const bool swap_x = ratio != nullptr && u1[i] < rate, swap_y = ratio != nullptr && u2[i] < rate;
        for (int b = threadIdx.x; b < bands; b += blockDim.x) {
            float x = normal[src * bands + b];
            float y = shadow[src * bands + b];
            // the reference draws the two decisions independently and builds the second pair from the ALREADY swapped
            // normal spectrum (normal_images_rand / ratio): reproduced
            if (swap_x) x = y * ratio[b];
            if (swap_y) y = x / ratio[b];
            out_x[i * bands + b] = x;
            out_y[i * bands + b] = y;
        }
    }
}

// NumPy's float32 -> integer cast as compiled for x86-64: cvttss2si to int32 (truncation toward zero; NaN, +-inf and
// values outside [-2^31, 2^31) give INT_MIN), then the low bits.  The generator ends in tanh, so values below casi_min
// (negative before the offset) do occur and wrap exactly like this.
__device__ __forceinline__ int32_t hypel_cvtt_i32(float v) {
    return (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : INT32_MIN;
}

template <typename T>
__device__ __forceinline__ T hypel_cast_out(float v) {
    return (T)hypel_cvtt_i32(v);
}
template <>
__device__ __forceinline__ float hypel_cast_out<float>(float v) {
    return v;
}

// float32 multiply, then float32 add, each rounded (NumPy evaluates the two operators separately): no fma
__device__ __forceinline__ float hypel_denorm(float x, float s, float o) {
#pragma clang fp contract(off)
    const float m = x * s;
    return m + o;
}

template <typename T>
struct Vec4Of;
template <>
struct Vec4Of<float> { using type = float4; };
template <>
struct Vec4Of<uint16_t> { using type = ushort4; };
template <>
struct Vec4Of<int16_t> { using type = short4; };
template <>
struct Vec4Of<uint8_t> { using type = uchar4; };

// VEC: rows of src and out start 4-element aligned (ld_src, ld_out multiples of 4, aligned bases).  One lane converts
// four neighbouring bands with one 16-byte load and one 4-element store; the bands % 4 remainder of a row goes through
// the scalar path of the row's last lane.  Without VEC one lane converts one element.
template <typename T, bool VEC>
__global__ void denorm_scatter_kernel(const float* __restrict__ src, int64_t ld_src, const int64_t* __restrict__ rows,
                                      int64_t n, int bands, const float* __restrict__ scale,
                                      const float* __restrict__ offset, T* __restrict__ out, int64_t ld_out) {
    const int per_row = VEC ? (bands + 3) >> 2 : bands;
    const int64_t total = n * per_row;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; item < total; item += stride) {
        const int64_t i = item / per_row;
        const int j = (int)(item - i * per_row);
        const float* s = src + i * ld_src;
        T* o = out + (rows ? rows[i] : i) * ld_out;
        if (VEC) {
            const int b0 = j << 2;
            if (b0 + 4 <= bands) {
                const float4 x = *reinterpret_cast<const float4*>(s + b0);
                const float4 sc = *reinterpret_cast<const float4*>(scale + b0);
                const float4 of = *reinterpret_cast<const float4*>(offset + b0);
                typename Vec4Of<T>::type r;
                r.x = hypel_cast_out<T>(hypel_denorm(x.x, sc.x, of.x));
                r.y = hypel_cast_out<T>(hypel_denorm(x.y, sc.y, of.y));
                r.z = hypel_cast_out<T>(hypel_denorm(x.z, sc.z, of.z));
                r.w = hypel_cast_out<T>(hypel_denorm(x.w, sc.w, of.w));
                *reinterpret_cast<typename Vec4Of<T>::type*>(o + b0) = r;
            } else {
                for (int b = b0; b < bands; ++b) o[b] = hypel_cast_out<T>(hypel_denorm(s[b], scale[b], offset[b]));
            }
        } else {
            o[j] = hypel_cast_out<T>(hypel_denorm(s[j], scale[j], offset[j]));
        }
    }
}

template <typename T>
int launch_denorm_scatter(const float* src, int64_t ld_src, const int64_t* rows, int64_t n, int bands,
                          const float* scale, const float* offset, void* out, int64_t ld_out, hipStream_t st) {
    T* o = static_cast<T*>(out);
    const bool vec = ld_src % 4 == 0 && ld_out % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)scale & 15) == 0 &&
                     ((uintptr_t)offset & 15) == 0 && ((uintptr_t)o % (4 * sizeof(T))) == 0;
    const int64_t work = n * (vec ? (bands + 3) / 4 : bands);
    const dim3 grid(hypel_grid_1d(work, 256, 256 * 64)), block(256);
    if (vec)
        hipLaunchKernelGGL((denorm_scatter_kernel<T, true>), grid, block, 0, st, src, ld_src, rows, n, bands, scale,
                           offset, o, ld_out);
    else
        hipLaunchKernelGGL((denorm_scatter_kernel<T, false>), grid, block, 0, st, src, ld_src, rows, n, bands, scale,
                           offset, o, ld_out);
    return 0;
}

// sRGB rendering of a raster.  A group of G lanes owns HSI_PIXELS = 4 neighbouring pixels at a time: the lanes load each
// pixel's span of bands contiguously (V neighbouring bands per lane, all the pixels' loads in flight together) and weigh
// them into partial X, Y, Z per pixel.  The reduction over the group transposes as it halves: at distance 8 a lane hands
// two of its four pixels to its partner and takes the partner's share of the other two, at distance 4 one of the two,
// so that after the distances 2 and 1 the four lanes 4 u .. 4 u + 3 hold the sums of pixel u (15 exchanges instead of
// the 12 per distance of a plain butterfly, which groups wider than 16 lanes still need above distance 8).  Lane
// 4 u + c then finishes colour channel c of pixel u and stores it.  table[b] = {offset, wx, wy, wz} of band band0 + b
// (weights already divided by the band's scale and by sum(ybar)); the first V entries of a lane stay in registers over
// the pixel loop, which covers the first pass over the span.
// The sums and the matrix are float64: linear sRGB is a difference of the three sums, float32 sums leave a dark channel
// of a bright pixel about 2e-6 off, and that moves trunc(255 * rgb) across an integer now and then (a 189-sample raster
// of the tests allows no such byte).  The curve itself is float32; for the byte output it only has to land within half a
// level, because levels[k], the smallest linear value whose float64 rendering reaches k, decides between k and k - 1.
constexpr int HSI_PIXELS = 4;

// V neighbouring bands of one pixel as they lie in memory (converted where they are weighed, so that the loads of a
// round cost few registers while they are in flight)
template <typename T, int V>
struct HsiBands { using type = typename Vec4Of<T>::type; };
template <typename T>
struct HsiBands<T, 1> { using type = T; };

template <typename T, int V>
__device__ __forceinline__ typename HsiBands<T, V>::type hsi_load(const T* p) {
    return *reinterpret_cast<const typename HsiBands<T, V>::type*>(p);
}

struct HsiXyz {
    double x, y, z;
};

__device__ __forceinline__ void hsi_weigh(double v, const double4 t, HsiXyz& a) {
    const double d = v - t.x;
    a.x = fma(d, t.y, a.x);
    a.y = fma(d, t.z, a.y);
    a.z = fma(d, t.w, a.z);
}

// one halving step of the reduction: the lane keeps `keep`, hands `give` to the lane at distance m and adds what that
// lane hands over in turn
template <int G>
__device__ __forceinline__ HsiXyz hsi_exchange(const HsiXyz keep, const HsiXyz give, int m) {
    return {keep.x + __shfl_xor(give.x, m, G), keep.y + __shfl_xor(give.y, m, G), keep.z + __shfl_xor(give.z, m, G)};
}

template <int V, typename B>
__device__ __forceinline__ void hsi_weigh_bands(const B v, const double4 (&t)[V], HsiXyz& a) {
    if constexpr (V == 4) {
        hsi_weigh((double)v.x, t[0], a);
        hsi_weigh((double)v.y, t[1], a);
        hsi_weigh((double)v.z, t[2], a);
        hsi_weigh((double)v.w, t[3], a);
    } else {
        hsi_weigh((double)v, t[0], a);
    }
}

// skimage's xyz2rgb on one channel's linear value, the sRGB transfer curve and the clip to [0, 1], in float32 on the
// hardware's log2 / exp2 (lin above the knee is a normal number): within 1e-6 of the curve
__device__ __forceinline__ float hsi_srgb_curve(float lin) {
    const float s = lin > 0.0031308f ? 1.055f * __builtin_amdgcn_exp2f((1.0f / 2.4f) * __builtin_amdgcn_logf(lin)) - 0.055f
                                     : 12.92f * lin;
    return fminf(fmaxf(s, 0.0f), 1.0f);
}

template <typename T, int G, int V>
__global__ void __launch_bounds__(256) hsi_to_srgb_kernel(const T* __restrict__ raster, int64_t ld_in, int64_t n, int span,
                                                          const double4* __restrict__ table,
                                                          const double* __restrict__ levels, void* __restrict__ out) {
    constexpr int U = HSI_PIXELS;
    static_assert(U == 4 && G >= 16 && G <= 64, "the reduction leaves pixel u in the lanes 4 u .. 4 u + 3");
    const int lane = threadIdx.x % G;
    const int nvec = span / V;  // whole V-band items of the span; the span % V bands left go one per lane
    const int rem = span - nvec * V;
    const double4 zero = make_double4(0.0, 0.0, 0.0, 0.0);  // a lane without a band weighs nothing
    double4 t0[V];
#pragma unroll
    for (int e = 0; e < V; ++e) t0[e] = lane < nvec ? table[lane * V + e] : zero;
    const double4 tr = lane < rem ? table[nvec * V + lane] : zero;
    const int64_t step = (int64_t)gridDim.x * (256 / G) * U;
    for (int64_t p0 = ((int64_t)blockIdx.x * (256 / G) + threadIdx.x / G) * U; p0 < n; p0 += step) {
        const T* row = raster + p0 * ld_in;
        const int live = n - p0 < U ? (int)(n - p0) : U;  // pixels of this round that exist
        using Bands = typename HsiBands<T, V>::type;
        HsiXyz a[U];
        Bands v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            a[u] = {0.0, 0.0, 0.0};
            v[u] = Bands{};
            if (lane < nvec && u < live) v[u] = hsi_load<T, V>(row + u * ld_in + lane * V);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) hsi_weigh_bands<V>(v[u], t0, a[u]);
        for (int j = lane + G; j < nvec; j += G) {
            double4 t[V];
#pragma unroll
            for (int e = 0; e < V; ++e) t[e] = table[j * V + e];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < live) v[u] = hsi_load<T, V>(row + u * ld_in + j * V);
#pragma unroll
            for (int u = 0; u < U; ++u) hsi_weigh_bands<V>(v[u], t, a[u]);
        }
        if (lane < rem) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < live) hsi_weigh((double)row[u * ld_in + nvec * V + lane], tr, a[u]);
        }
#pragma unroll
        for (int m = G / 2; m >= 16; m >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] = hsi_exchange<G>(a[u], a[u], m);
        }
        const bool up8 = (lane & 8) != 0, up4 = (lane & 4) != 0;
        const HsiXyz b0 = hsi_exchange<G>(up8 ? a[2] : a[0], up8 ? a[0] : a[2], 8);  // pixel 2 h
        const HsiXyz b1 = hsi_exchange<G>(up8 ? a[3] : a[1], up8 ? a[1] : a[3], 8);  // pixel 2 h + 1, h = bit 3
        HsiXyz s = hsi_exchange<G>(up4 ? b1 : b0, up4 ? b0 : b1, 4);               // pixel 2 h + bit 2
        s = hsi_exchange<G>(s, s, 2);
        s = hsi_exchange<G>(s, s, 1);
        const int u = lane >> 2, c = lane & 3;
        if (u < live && c < 3) {
            const double px = s.x, py = s.y, pz = s.z;
            // row c of the inverse of skimage's xyz_from_rgb [[0.412453, 0.357580, 0.180423], [0.212671, 0.715160,
            // 0.072169], [0.019334, 0.119193, 0.950227]]
            const double mx = c == 0 ? 3.240481343200526 : (c == 1 ? -0.9692549499965682 : 0.05564663913517716);
            const double my = c == 0 ? -1.5371515162713185 : (c == 1 ? 1.8759900014898907 : -0.20404133836651123);
            const double mz = c == 0 ? -0.4985363261688878 : (c == 1 ? 0.04155592655829284 : 1.0573110696453443);
            const double lin = mx * px + my * py + mz * pz;
            const bool finite = lin - lin == 0.0;  // only non-finite input makes it otherwise: rendered as 0
            const float rgb = finite ? hsi_srgb_curve((float)lin) : 0.0f;
            const int64_t o = (p0 + u) * 3 + c;
            if (levels == nullptr) {
                static_cast<float*>(out)[o] = rgb;
            } else {
                const int k = (int)rintf(255.0f * rgb);  // rgb in [0, 1]; levels[0] = -inf
                static_cast<uint8_t*>(out)[o] = (uint8_t)((finite && lin >= levels[k]) ? k : (k > 0 ? k - 1 : 0));
            }
        }
    }
}

template <typename T, int G, int V>
void launch_hsi_to_srgb_gv(const T* raster, int64_t ld_in, int64_t n, int span, const double* table, const double* levels,
                           void* out, hipStream_t st) {
    const dim3 grid(hypel_grid_1d(n, 256 / G * HSI_PIXELS, 256 * 32)), block(256);
    hipLaunchKernelGGL((hsi_to_srgb_kernel<T, G, V>), grid, block, 0, st, raster, ld_in, n, span,
                       reinterpret_cast<const double4*>(table), levels, out);
}

template <typename T, int V>
void launch_hsi_to_srgb_v(const T* raster, int64_t ld_in, int64_t n, int span, const double* table, const double* levels,
                          void* out, hipStream_t st) {
    // lanes per group: enough to cover the span in four passes.  Measured on 349 x 1905 pixels, one, two and four
    // passes: 120 / 91 / 92 us at a span of 68 bands, 320 / 320 / 250 us at 360; no difference at 52 bands and below
    const int items = ((span + V - 1) / V + 3) / 4;
    if (items <= 16)
        launch_hsi_to_srgb_gv<T, 16, V>(raster, ld_in, n, span, table, levels, out, st);
    else if (items <= 32)
        launch_hsi_to_srgb_gv<T, 32, V>(raster, ld_in, n, span, table, levels, out, st);
    else
        launch_hsi_to_srgb_gv<T, 64, V>(raster, ld_in, n, span, table, levels, out, st);
}

// four bands per lane when every pixel's span starts on a four-element boundary, one band per lane otherwise
template <typename T>
void launch_hsi_to_srgb(const void* raster, int64_t ld_in, int64_t n, int band0, int span, const double* table,
                        const double* levels, void* out, hipStream_t st) {
    const T* r = static_cast<const T*>(raster) + band0;
    if (ld_in % 4 == 0 && (uintptr_t)r % (4 * sizeof(T)) == 0)
        launch_hsi_to_srgb_v<T, 4>(r, ld_in, n, span, table, levels, out, st);
    else
        launch_hsi_to_srgb_v<T, 1>(r, ld_in, n, span, table, levels, out, st);
}

}  // namespace

extern "C" int hypel_gather_pairs_f32(const float* normal, const float* shadow, const int64_t* idx, int64_t n, int32_t bands,
                                      const float* ratio, const float* u1, const float* u2, float rate, float* out_x,
                                      float* out_y, hypel_stream_t stream) {
    HYPEL_REQUIRE(normal && shadow && idx && out_x && out_y && n > 0 && bands > 0, "hypel_gather_pairs_f32");
    HYPEL_REQUIRE(ratio == nullptr || (u1 && u2), "hypel_gather_pairs_f32");
    const int block = bands >= 192 ? 256 : (bands >= 96 ? 128 : 64);
    hipLaunchKernelGGL(gather_pairs_kernel, dim3(hypel_grid_1d(n, 1, 256 * 32)), dim3(block), 0, ST, normal, shadow, idx, n,
                       bands, ratio, u1, u2, rate, out_x, out_y);
    HYPEL_CHECK_LAUNCH("hypel_gather_pairs_f32");
    return 0;
}

extern "C" int hypel_gather_patches_f32(const float* casi, const float* lidar, int64_t hp, int64_t wp, int32_t cc,
                                        int32_t cl, const int32_t* points, int64_t n, int32_t p, float* out,
                                        hypel_stream_t stream) {
    HYPEL_REQUIRE(casi && points && out && n > 0 && p > 0 && cc > 0 && cl >= 0 && hp >= p && wp >= p,
                  "hypel_gather_patches_f32");
    HYPEL_REQUIRE(cl == 0 || lidar, "hypel_gather_patches_f32");
    const int c = cc + cl;
    const int block = c >= 192 ? 256 : (c >= 96 ? 128 : 64);
    hipLaunchKernelGGL(gather_patches_kernel, dim3(hypel_grid_1d(n * p * p, 1, 256 * 32)), dim3(block), 0, ST, casi,
                       lidar, wp, cc, cl, points, n, p, out);
    HYPEL_CHECK_LAUNCH("hypel_gather_patches_f32");
    return 0;
}

extern "C" int hypel_gather_patches_2x_f32(const float* casi, const float* lidar, int64_t casi_wp, int64_t lidar_wp,
                                           int32_t cc, int32_t cl, int32_t neighborhood, const int32_t* points,
                                           int64_t n, int32_t p, float* out, hypel_stream_t stream) {
    HYPEL_REQUIRE(casi && lidar && points && out && n > 0 && p > 0 && cc > 0 && cl > 0 && neighborhood >= 0,
                  "hypel_gather_patches_2x_f32");
    const int c = cc + cl;
    const int block = c >= 192 ? 256 : (c >= 96 ? 128 : 64);
    hipLaunchKernelGGL(gather_patches_2x_kernel, dim3(hypel_grid_1d(n * p * p, 1, 256 * 32)), dim3(block), 0, ST, casi,
                       lidar, casi_wp, lidar_wp, cc, cl, neighborhood, points, n, p, out);
    HYPEL_CHECK_LAUNCH("hypel_gather_patches_2x_f32");
    return 0;
}

extern "C" int hypel_augment_patches_f32(const float* x, const int64_t* idx, int64_t n, int32_t p, int32_t c,
                                         const int32_t* rot_k, const uint8_t* shadow_pick, const float* shadow_ratio,
                                         const float* shadow_alt, const uint8_t* flip_lr, const uint8_t* flip_ud,
                                         const float* delta, float* out, hypel_stream_t stream) {
    HYPEL_REQUIRE(x && out && x != out && n > 0 && p > 0 && c > 0, "hypel_augment_patches_f32");
    HYPEL_REQUIRE(!shadow_pick || shadow_ratio || shadow_alt, "hypel_augment_patches_f32");
    HYPEL_REQUIRE(!(shadow_ratio && shadow_alt), "hypel_augment_patches_f32");  // one shadow operator per call
    const int block = c >= 192 ? 256 : (c >= 96 ? 128 : 64);
    hipLaunchKernelGGL(augment_patches_kernel, dim3(hypel_grid_1d(n * p * p, 1, 256 * 32)), dim3(block), 0, ST, x, idx,
                       n, p, c, rot_k, shadow_pick, shadow_ratio, shadow_alt, flip_lr, flip_ud, delta, out);
    HYPEL_CHECK_LAUNCH("hypel_augment_patches_f32");
    return 0;
}

extern "C" int hypel_argmax_scatter(const float* logits, int64_t ld, int64_t n, int32_t c, const int32_t* points,
                                    uint8_t* raster, int64_t raster_w, hypel_stream_t stream) {
    HYPEL_REQUIRE(logits && points && raster && n > 0 && c > 0 && c <= 256 && raster_w > 0, "hypel_argmax_scatter");
    hipLaunchKernelGGL(argmax_scatter_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, ST, logits, ld, n, c,
                       points, raster, raster_w);
    HYPEL_CHECK_LAUNCH("hypel_argmax_scatter");
    return 0;
}

extern "C" int hypel_denorm_scatter(const float* src, int64_t ld_src, const int64_t* rows, int64_t n, int32_t bands,
                                    const float* scale, const float* offset, int32_t out_dtype, void* out,
                                    int64_t ld_out, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && scale && offset && out && n > 0 && bands > 0 && ld_src >= bands && ld_out >= bands,
                  "hypel_denorm_scatter");
    switch (out_dtype) {
        case HYPEL_DTYPE_F32: launch_denorm_scatter<float>(src, ld_src, rows, n, bands, scale, offset, out, ld_out, ST); break;
        case HYPEL_DTYPE_U16: launch_denorm_scatter<uint16_t>(src, ld_src, rows, n, bands, scale, offset, out, ld_out, ST); break;
        case HYPEL_DTYPE_I16: launch_denorm_scatter<int16_t>(src, ld_src, rows, n, bands, scale, offset, out, ld_out, ST); break;
        case HYPEL_DTYPE_U8: launch_denorm_scatter<uint8_t>(src, ld_src, rows, n, bands, scale, offset, out, ld_out, ST); break;
        default: hypel_set_error("hypel_denorm_scatter: unsupported out_dtype %d", (int)out_dtype); return -1;
    }
    HYPEL_CHECK_LAUNCH("hypel_denorm_scatter");
    return 0;
}

extern "C" int hypel_hsi_to_srgb(const void* raster, int32_t in_dtype, int64_t ld_in, int64_t n_pixels, int32_t bands,
                                 int32_t band0, int32_t span, const double* table, const double* levels,
                                 int32_t out_mode, void* out, hypel_stream_t stream) {
    HYPEL_REQUIRE(raster && table && out && n_pixels > 0 && bands > 0 && ld_in >= bands, "hypel_hsi_to_srgb");
    HYPEL_REQUIRE(band0 >= 0 && span > 0 && span <= bands - band0, "hypel_hsi_to_srgb");
    HYPEL_REQUIRE(((uintptr_t)table & 31) == 0, "hypel_hsi_to_srgb");
    HYPEL_REQUIRE((out_mode == HYPEL_RGB_U8 && levels && ((uintptr_t)levels & 7) == 0) ||
                      (out_mode == HYPEL_RGB_F32 && ((uintptr_t)out & 3) == 0),
                  "hypel_hsi_to_srgb");
    if (out_mode == HYPEL_RGB_F32) levels = nullptr;
    switch (in_dtype) {
        case HYPEL_DTYPE_F32:
            HYPEL_REQUIRE(((uintptr_t)raster & 3) == 0, "hypel_hsi_to_srgb");
            launch_hsi_to_srgb<float>(raster, ld_in, n_pixels, band0, span, table, levels, out, ST);
            break;
        case HYPEL_DTYPE_U16:
            HYPEL_REQUIRE(((uintptr_t)raster & 1) == 0, "hypel_hsi_to_srgb");
            launch_hsi_to_srgb<uint16_t>(raster, ld_in, n_pixels, band0, span, table, levels, out, ST);
            break;
        case HYPEL_DTYPE_I16:
            HYPEL_REQUIRE(((uintptr_t)raster & 1) == 0, "hypel_hsi_to_srgb");
            launch_hsi_to_srgb<int16_t>(raster, ld_in, n_pixels, band0, span, table, levels, out, ST);
            break;
        case HYPEL_DTYPE_U8: launch_hsi_to_srgb<uint8_t>(raster, ld_in, n_pixels, band0, span, table, levels, out, ST); break;
        default: hypel_set_error("hypel_hsi_to_srgb: unsupported in_dtype %d", (int)in_dtype); return -1;
    }
    HYPEL_CHECK_LAUNCH("hypel_hsi_to_srgb");
    return 0;
}
