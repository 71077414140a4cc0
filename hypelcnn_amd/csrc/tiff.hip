// TIFF layouts: from "the file's bytes are in HBM" to the raster [h][w][spp] scene.hip reads (common/tiff_io.py).
//   * tiff_unpack   : LZW / PackBits segments -> their decoded bytes, one wavefront per segment
//   * tiff_assemble : predictor undo, byte swap, de-tiling (edge tiles and the short last strip clipped), plane
//                     interleave; one wavefront per segment row (or per piece of one when nothing is accumulated)
// Both read the file through byte loads: a strip may start at any offset, and a fault here would cost more than the
// instructions do -- the floor is one read of the decoded bytes plus one write of the raster, and the upload of the
// file in front of these launches is two orders of magnitude slower than either.
//
// LZW without a string table: a string added to the table is always "the previous string plus one byte", and the
// previous string has just been written, directly in front of the byte that extends it.  So an entry is (position in
// the output, length), decoding a code is a forward copy from earlier output done by the 64 lanes, and code ==
// next-free (the string that ends in its own first byte) is the same copy read with period length - 1.  Only the
// code stream is serial: every lane decodes every code, from a 256-byte window of the stream held one word per lane.
// The output is built in a 16 KiB ring in LDS and reaches the buffer 1 KiB at a time (a store per string would put a
// few bytes into the same cache line over and over); a table fills after 3836 strings, so nearly every copy finds
// its source in the ring, and an older source is read back from the buffer.
#include "common.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int WAVE = 64;
// bytes of recent output an LZW segment keeps in LDS (a power of two).  With the 24 KiB table a block holds 40 KiB, so
// four segments decode per CU (160 KiB), one per SIMD: 1024 at once.  A table refills after 3836 strings, of a few
// bytes each in a scene: 16 KiB hold nearly every source, and the rest is read back from the output buffer.
constexpr int LZW_RING = 16384;
constexpr int LZW_FLUSH = 1024;  // the ring reaches the output buffer in pieces of this size: whole lines, not strings

// ------------------------------------------------------------------------------------------------ unpack
struct Window {
    uint32_t word;  // lane l: bytes base + 4 l .. + 3 of the segment's stream, the first in the low bits
    int64_t base;
};

__device__ __forceinline__ void window_fill(Window& win, const uint8_t* __restrict__ in, int64_t len, int64_t at,
                                            int lane) {
    win.base = at;
    const int64_t p = at + 4 * lane;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p + k < len) v |= (uint32_t)in[p + k] << (8 * k);
    win.word = v;
}

// byte `idx` of the stream (0 past its end: the callers test the length first); idx is the same in every lane, so the
// word comes by v_readlane and the result is scalar: the decoders' bookkeeping stays in scalar registers and
// instructions, which is what a segment's one wave -- often alone on its SIMD -- has to spare
__device__ __forceinline__ uint32_t window_byte(Window& win, const uint8_t* __restrict__ in, int64_t len, int64_t idx,
                                                int lane) {
    if (idx < win.base || idx >= win.base + 4 * WAVE) window_fill(win, in, len, idx, lane);
    const int rel = (int)(idx - win.base);
    return ((uint32_t)__builtin_amdgcn_readlane((int)win.word, rel >> 2) >> (8 * (rel & 3))) & 255u;
}

__device__ __forceinline__ bool seg_range_ok(const hypel_tiff_seg_t& g, int64_t src_bytes, int64_t dst_bytes) {
    return g.src_off >= 0 && g.src_len >= 0 && g.src_len <= src_bytes && g.src_off <= src_bytes - g.src_len &&
           g.dst_off >= 0 && g.dst_len >= 0 && g.dst_len <= dst_bytes && g.dst_off <= dst_bytes - g.dst_len &&
           g.dst_len <= 0xffffffffll;  // table positions are 32 bits
}

// output bytes [a, b) of a segment from the ring to the buffer: whole words where the addresses allow it
__device__ __forceinline__ void lzw_flush(uint8_t* out, const uint8_t* ring, int64_t a, int64_t b, int lane) {
    __builtin_amdgcn_wave_barrier();
    if ((((uintptr_t)out | (uintptr_t)a | (uintptr_t)b) & 3) == 0) {
        for (int64_t p = a + 4 * lane; p < b; p += 4 * WAVE)
            *(uint32_t*)(out + p) = *(const uint32_t*)(ring + (p & (LZW_RING - 1)));
    } else {
        for (int64_t p = a + lane; p < b; p += WAVE) out[p] = ring[p & (LZW_RING - 1)];
    }
    __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(WAVE) lzw_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                   const hypel_tiff_seg_t* __restrict__ segs, uint8_t* dst,
                                                   int64_t dst_bytes, int32_t* __restrict__ status) {
    __shared__ uint32_t t_pos[4096];
    __shared__ uint16_t t_len[4096];
    __shared__ __attribute__((aligned(16))) uint8_t ring[LZW_RING];  // output byte p at ring[p % LZW_RING]
    const int s = blockIdx.x, lane = threadIdx.x;
    const hypel_tiff_seg_t g = segs[s];
    if (!seg_range_ok(g, src_bytes, dst_bytes)) {
        if (lane == 0) status[s] = HYPEL_TIFF_BAD_RANGE;
        return;
    }
    const uint8_t* in = src + g.src_off;
    uint8_t* out = dst + g.dst_off;
    const int64_t len = g.src_len, in_bits = g.src_len * 8, need = g.dst_len;
    Window win;
    window_fill(win, in, len, 0, lane);
    int64_t bitpos = 0, done = 0, prev_pos = 0, flushed = 0;
    int width = 9, next = 258, prev_len = 0;  // prev_len 0: no string yet since the last Clear
    int st = HYPEL_TIFF_OK;
    while (done < need) {
        if (bitpos + width > in_bits) {
            st = HYPEL_TIFF_TRUNCATED;
            break;
        }
        const int64_t at = bitpos >> 3;
        const uint32_t b0 = window_byte(win, in, len, at, lane), b1 = window_byte(win, in, len, at + 1, lane),
                       b2 = window_byte(win, in, len, at + 2, lane);
        const uint32_t code = (((b0 << 16) | (b1 << 8) | b2) >> (24 - (int)(bitpos & 7) - width)) & ((1u << width) - 1u);
        bitpos += width;
        if (code == 257u) break;
        if (code == 256u) {
            width = 9;
            next = 258;
            prev_len = 0;
            continue;
        }
        int cur_len = 1;
        if (code < 256u) {
            if (lane == 0) ring[done & (LZW_RING - 1)] = (uint8_t)code;
        } else {
            if (prev_len == 0) {
                st = HYPEL_TIFF_BAD_FIRST;
                break;
            }
            int64_t from;
            int period;
            if ((int)code < next) {  // (every lane read the same entry: keep it scalar)
                from = (uint32_t)__builtin_amdgcn_readfirstlane((int)t_pos[code]);
                cur_len = period = __builtin_amdgcn_readfirstlane((int)t_len[code]);
            } else if ((int)code == next) {
                from = prev_pos;
                period = prev_len;
                cur_len = prev_len + 1;
            } else {
                st = HYPEL_TIFF_BAD_CODE;
                break;
            }
            const int n = need - done < cur_len ? (int)(need - done) : cur_len;
            // from + period <= done: the source lies in front of what is written here
            if (from >= done + n - LZW_RING) {
                // the usual case: the source is still in the ring, and none of it is overwritten by this string.  A
                // wave's LDS accesses execute in order, so what its lanes stored so far is what they read now.
                __builtin_amdgcn_wave_barrier();
                for (int i = lane; i < n; i += WAVE)
                    ring[(done + i) & (LZW_RING - 1)] = ring[(from + (i >= period ? i - period : i)) & (LZW_RING - 1)];
                __builtin_amdgcn_wave_barrier();
            } else {
                // older than the ring: flushed long ago (the flush lags by less than LZW_FLUSH + one string)
                __syncthreads();  // one wave per block: its earlier stores to `out` are what its lanes read now
                for (int i = lane; i < n; i += WAVE)
                    ring[(done + i) & (LZW_RING - 1)] = out[from + (i >= period ? i - period : i)];
            }
        }
        if (prev_len != 0 && next < 4096) {  // previous string + the first byte of this one: it follows it in `out`
            t_pos[next] = (uint32_t)prev_pos;
            t_len[next] = (uint16_t)(prev_len + 1);
            ++next;
        }
        prev_pos = done;
        prev_len = cur_len;
        done += cur_len;  // past `need` only when the string was clipped: the loop ends then
        while (flushed + LZW_FLUSH <= (done < need ? done : need)) {
            lzw_flush(out, ring, flushed, flushed + LZW_FLUSH, lane);
            flushed += LZW_FLUSH;
        }
        width = 9 + (next >= 511) + (next >= 1023) + (next >= 2047);
    }
    lzw_flush(out, ring, flushed, done < need ? done : need, lane);  // what was decoded, also in front of a fault
    if (st == HYPEL_TIFF_OK && done < need) st = HYPEL_TIFF_TRUNCATED;  // EOI in front of the segment's end
    if (lane == 0) status[s] = st;
}

__global__ void __launch_bounds__(WAVE) packbits_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                        const hypel_tiff_seg_t* __restrict__ segs,
                                                        uint8_t* __restrict__ dst, int64_t dst_bytes,
                                                        int32_t* __restrict__ status) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const hypel_tiff_seg_t g = segs[s];
    if (!seg_range_ok(g, src_bytes, dst_bytes)) {
        if (lane == 0) status[s] = HYPEL_TIFF_BAD_RANGE;
        return;
    }
    const uint8_t* in = src + g.src_off;
    uint8_t* out = dst + g.dst_off;
    const int64_t len = g.src_len, need = g.dst_len;
    Window win;
    window_fill(win, in, len, 0, lane);
    int64_t at = 0, done = 0;
    int st = HYPEL_TIFF_OK;
    while (done < need) {
        if (at >= len) {
            st = HYPEL_TIFF_TRUNCATED;
            break;
        }
        const int n = (int)window_byte(win, in, len, at, lane);
        ++at;
        if (n < 128) {
            const int64_t avail = len - at < n + 1 ? len - at : n + 1;
            const int64_t m = need - done < avail ? need - done : avail;
            for (int64_t i = lane; i < m; i += WAVE) out[done + i] = in[at + i];
            done += m;
            at += n + 1;
            if (avail < n + 1 && done < need) {
                st = HYPEL_TIFF_TRUNCATED;
                break;
            }
        } else if (n > 128) {
            if (at >= len) {
                st = HYPEL_TIFF_TRUNCATED;
                break;
            }
            const uint8_t v = (uint8_t)window_byte(win, in, len, at, lane);
            ++at;
            const int64_t m = need - done < 257 - n ? need - done : 257 - n;
            for (int64_t i = lane; i < m; i += WAVE) out[done + i] = v;
            done += m;
        }
    }
    if (lane == 0) status[s] = st;
}

// ------------------------------------------------------------------------------------------------ assemble
struct TiffGeom {
    int64_t h, w, src_bytes, row_bytes;
    int spp, sps;  // samples per pixel of the raster / of a segment (1 in a planar file)
    int seg_rows, seg_cols, segs_across, segs_down, planes;
    int from_decoded, swap;
};

// sample `idx` of a segment row as its bits in native order
template <int ITEM>
__device__ __forceinline__ uint32_t load_sample(const uint8_t* __restrict__ row, int64_t idx, int swap) {
    const uint8_t* p = row + idx * ITEM;
    if (ITEM == 1) return p[0];
    if (ITEM == 2) {
        const uint32_t a = p[0], b = p[1];
        return swap ? (a << 8) | b : a | (b << 8);
    }
    const uint32_t a = p[0], b = p[1], c = p[2], d = p[3];
    return swap ? (a << 24) | (b << 16) | (c << 8) | d : a | (b << 8) | (c << 16) | (d << 24);
}

// predictor 3: byte k of sample idx is byte idx of the row's k-th plane of n bytes, most significant plane first
__device__ __forceinline__ uint32_t load_planes(const uint8_t* __restrict__ row, int64_t idx, int64_t n) {
    return ((uint32_t)row[idx] << 24) | ((uint32_t)row[n + idx] << 16) | ((uint32_t)row[2 * n + idx] << 8) |
           (uint32_t)row[3 * n + idx];
}

template <int ITEM>
__device__ __forceinline__ void store_sample(void* __restrict__ out, int64_t idx, uint32_t v) {
    if (ITEM == 1) ((uint8_t*)out)[idx] = (uint8_t)v;
    if (ITEM == 2) ((uint16_t*)out)[idx] = (uint16_t)v;
    if (ITEM == 4) ((uint32_t*)out)[idx] = v;
}

// predictor 2 adds modulo the sample width (the store truncates); predictor 3 adds the four bytes separately
template <int PRED>
__device__ __forceinline__ uint32_t pred_add(uint32_t a, uint32_t b) {
    if (PRED == 3) return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
    return a + b;
}

// predictor 3 accumulates over the whole row of bytes, plane after plane: plane k of a residue class starts from the
// sums of the planes in front of it.  tot: the four per-plane sums of the class (plane 0 in the high byte).
__device__ __forceinline__ uint32_t plane_carry(uint32_t tot) {
    const uint32_t t0 = tot >> 24, t1 = (tot >> 16) & 255u, t2 = (tot >> 8) & 255u;
    return ((t0 & 255u) << 16) | (((t0 + t1) & 255u) << 8) | ((t0 + t1 + t2) & 255u);
}

struct RowRef {
    const uint8_t* row;
    int64_t y, x0;
    int plane;
    bool live;
};

// segment row `row_id` (segment-major): where it lies, where it goes, and whether there is anything to do
__device__ __forceinline__ RowRef locate_row(const uint8_t* __restrict__ src, const hypel_tiff_seg_t* __restrict__ segs,
                                             const TiffGeom& g, int64_t row_id) {
    RowRef r;
    const int64_t s = row_id / g.seg_rows;
    const int rr = (int)(row_id - s * g.seg_rows);
    const int64_t per_plane = (int64_t)g.segs_across * g.segs_down;
    r.plane = (int)(s / per_plane);
    const int64_t rest = s - r.plane * per_plane;
    const int64_t sy = rest / g.segs_across, sx = rest - sy * g.segs_across;
    r.y = sy * g.seg_rows + rr;
    r.x0 = sx * g.seg_cols;
    r.live = false;
    r.row = src;
    if (r.y >= g.h) return r;  // rows of a bottom tile below the image; what the short last strip does not store
    const hypel_tiff_seg_t seg = segs[s];
    const int64_t base = g.from_decoded ? seg.dst_off : seg.src_off, len = g.from_decoded ? seg.dst_len : seg.src_len;
    const int64_t at = (int64_t)rr * g.row_bytes;
    if (base < 0 || len < 0 || at + g.row_bytes > len || base > g.src_bytes - at - g.row_bytes) return r;
    r.row = src + base + at;
    r.live = true;
    return r;
}

constexpr int THREADS = 256, WAVES = THREADS / WAVE;
constexpr int NARROW_SPAN = 8;  // chunks of 64 samples per wave where nothing is accumulated
constexpr int WIDE_SPAN = 32;   // pixels per wave there

// sps <= 64.  A wave walks a segment row in chunks of P = 64 / sps whole pixels, lane = (pixel of the chunk, sample):
// consecutive lanes on consecutive samples.  The predictor is a scan over the lanes with stride sps and a carry from
// the last pixel of the previous chunk; lanes past the row's end add 0, so the carry survives a short last chunk.
template <int ITEM, int PRED>
__global__ void __launch_bounds__(THREADS) assemble_narrow_kernel(const uint8_t* __restrict__ src,
                                                                  const hypel_tiff_seg_t* __restrict__ segs, TiffGeom g,
                                                                  int64_t n_rows, int parts, void* __restrict__ out) {
    const int lane = threadIdx.x % WAVE;
    const int64_t wid = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
    const int64_t row_id = wid / parts;
    const int part = (int)(wid - row_id * parts);
    if (row_id >= n_rows) return;
    const RowRef r = locate_row(src, segs, g, row_id);
    if (!r.live) return;
    const int sps = g.sps, P = WAVE / sps, L = P * sps;
    const int q = lane % sps, pl = lane / sps;
    const int chunks = (g.seg_cols + P - 1) / P;
    const int c0 = PRED > 1 ? 0 : part * NARROW_SPAN;
    const int c1 = PRED > 1 ? chunks : (c0 + NARROW_SPAN < chunks ? c0 + NARROW_SPAN : chunks);
    const int64_t n = (int64_t)g.seg_cols * sps;
    const int carry_lane = L - sps + q;
    const int out_q = g.planes > 1 ? r.plane : q;
    uint32_t prev = 0;
    for (int pass = PRED == 3 ? 0 : 1; pass < 2; ++pass) {  // predictor 3: the per-plane sums first
        for (int c = c0; c < c1; ++c) {
            const int p = c * P + pl;
            const bool valid = lane < L && p < g.seg_cols;
            uint32_t v = 0;
            if (valid) v = PRED == 3 ? load_planes(r.row, (int64_t)p * sps + q, n) : load_sample<ITEM>(r.row, (int64_t)p * sps + q, g.swap);
            if (PRED > 1) {
                for (int off = sps; off < L; off <<= 1) {
                    const uint32_t t = (uint32_t)__shfl_up((int)v, off);
                    if (lane >= off) v = pred_add<PRED>(v, t);
                }
                v = pred_add<PRED>(v, (uint32_t)__shfl((int)prev, carry_lane));
                prev = v;
            }
            if (pass == 1 && valid && r.x0 + p < g.w) store_sample<ITEM>(out, ((r.y * g.w) + r.x0 + p) * g.spp + out_q, v);
        }
        if (PRED == 3 && pass == 0) prev = plane_carry((uint32_t)__shfl((int)prev, carry_lane));
    }
}

// sps > 64.  A wave takes 64 consecutive samples of the pixel and walks the row pixel by pixel with the running sum
// in a register: every load and store is 64 consecutive samples.
template <int ITEM, int PRED>
__global__ void __launch_bounds__(THREADS) assemble_wide_kernel(const uint8_t* __restrict__ src,
                                                                const hypel_tiff_seg_t* __restrict__ segs, TiffGeom g,
                                                                int64_t n_rows, int slices, int parts,
                                                                void* __restrict__ out) {
    const int lane = threadIdx.x % WAVE;
    int64_t wid = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
    const int part = (int)(wid % parts);
    wid /= parts;
    const int slice = (int)(wid % slices);
    const int64_t row_id = wid / slices;
    if (row_id >= n_rows) return;
    const RowRef r = locate_row(src, segs, g, row_id);
    if (!r.live) return;
    const int sps = g.sps, q = slice * WAVE + lane;
    if (q >= sps) return;
    const int p0 = PRED > 1 ? 0 : part * WIDE_SPAN;
    int p1 = PRED > 1 ? g.seg_cols : (p0 + WIDE_SPAN < g.seg_cols ? p0 + WIDE_SPAN : g.seg_cols);
    const int64_t n = (int64_t)g.seg_cols * sps;
    uint32_t run = 0;
    if (PRED == 3) {
        for (int p = p0; p < p1; ++p) run = pred_add<3>(run, load_planes(r.row, (int64_t)p * sps + q, n));
        run = plane_carry(run);
    }
    if (r.x0 + p1 > g.w && PRED < 2) p1 = (int)(g.w - r.x0);  // nothing is carried: the padding columns are not read
#pragma unroll 4
    for (int p = p0; p < p1; ++p) {
        uint32_t v = PRED == 3 ? load_planes(r.row, (int64_t)p * sps + q, n) : load_sample<ITEM>(r.row, (int64_t)p * sps + q, g.swap);
        if (PRED > 1) v = run = pred_add<PRED>(run, v);
        if (r.x0 + p < g.w) store_sample<ITEM>(out, ((r.y * g.w) + r.x0 + p) * g.spp + q, v);
    }
}

// How a launch is cut into waves: computed once, checked by the entry point, used by the launch.
struct AssemblePlan {
    int slices, parts;  // 64-sample slices of a pixel (1 on the narrow path); pieces of a row
    int64_t blocks;
};

AssemblePlan plan_assemble(const TiffGeom& g, int64_t n_rows, int predictor) {
    AssemblePlan p;
    if (g.sps <= WAVE) {
        const int P = WAVE / g.sps, chunks = (g.seg_cols + P - 1) / P;
        p.slices = 1;
        p.parts = predictor > 1 ? 1 : (chunks + NARROW_SPAN - 1) / NARROW_SPAN;
    } else {
        p.slices = (g.sps + WAVE - 1) / WAVE;
        p.parts = predictor > 1 ? 1 : (g.seg_cols + WIDE_SPAN - 1) / WIDE_SPAN;
    }
    p.blocks = (n_rows * p.slices * p.parts + WAVES - 1) / WAVES;
    return p;
}

template <int ITEM, int PRED>
void launch_assemble(const uint8_t* src, const hypel_tiff_seg_t* segs, const TiffGeom& g, int64_t n_rows,
                     const AssemblePlan& p, void* out, hipStream_t st) {
    if (g.sps <= WAVE)
        hipLaunchKernelGGL((assemble_narrow_kernel<ITEM, PRED>), dim3((unsigned)p.blocks), dim3(THREADS), 0, st, src,
                           segs, g, n_rows, p.parts, out);
    else
        hipLaunchKernelGGL((assemble_wide_kernel<ITEM, PRED>), dim3((unsigned)p.blocks), dim3(THREADS), 0, st, src,
                           segs, g, n_rows, p.slices, p.parts, out);
}

}  // namespace

extern "C" int hypel_tiff_unpack(const uint8_t* src, int64_t src_bytes, const hypel_tiff_seg_t* segs, int32_t n_segs,
                                 int32_t codec, uint8_t* dst, int64_t dst_bytes, int32_t* status,
                                 hypel_stream_t stream) {
    HYPEL_REQUIRE(src && segs && dst && status, "hypel_tiff_unpack");
    HYPEL_REQUIRE(src_bytes > 0 && dst_bytes > 0 && n_segs > 0, "hypel_tiff_unpack");
    HYPEL_REQUIRE(codec == HYPEL_TIFF_LZW || codec == HYPEL_TIFF_PACKBITS, "hypel_tiff_unpack");
    if (codec == HYPEL_TIFF_LZW)
        hipLaunchKernelGGL(lzw_kernel, dim3(n_segs), dim3(WAVE), 0, ST, src, src_bytes, segs, dst, dst_bytes, status);
    else
        hipLaunchKernelGGL(packbits_kernel, dim3(n_segs), dim3(WAVE), 0, ST, src, src_bytes, segs, dst, dst_bytes,
                           status);
    HYPEL_CHECK_LAUNCH("hypel_tiff_unpack");
    return 0;
}

extern "C" int hypel_tiff_assemble(const uint8_t* src, int64_t src_bytes, const hypel_tiff_seg_t* segs, int32_t n_segs,
                                   int32_t from_decoded, int64_t h, int64_t w, int32_t spp, int32_t item,
                                   int32_t seg_rows, int32_t seg_cols, int32_t segs_across, int32_t planes,
                                   int32_t predictor, int32_t swap, void* out, hypel_stream_t stream) {
    HYPEL_REQUIRE(src && segs && out, "hypel_tiff_assemble");
    HYPEL_REQUIRE(src_bytes > 0 && n_segs > 0, "hypel_tiff_assemble");
    HYPEL_REQUIRE(h > 0 && w > 0 && spp > 0 && h < (1ll << 31) && w < (1ll << 31), "hypel_tiff_assemble");
    HYPEL_REQUIRE(item == 1 || item == 2 || item == 4, "hypel_tiff_assemble");
    HYPEL_REQUIRE(predictor == 1 || predictor == 2 || (predictor == 3 && item == 4), "hypel_tiff_assemble");
    HYPEL_REQUIRE((from_decoded == 0 || from_decoded == 1) && (swap == 0 || swap == 1), "hypel_tiff_assemble");
    HYPEL_REQUIRE(seg_rows > 0 && seg_cols > 0 && segs_across > 0, "hypel_tiff_assemble");
    HYPEL_REQUIRE(planes == 1 || planes == spp, "hypel_tiff_assemble");
    HYPEL_REQUIRE((uintptr_t)out % (uintptr_t)item == 0, "hypel_tiff_assemble");
    TiffGeom g;
    g.h = h;
    g.w = w;
    g.src_bytes = src_bytes;
    g.spp = spp;
    g.sps = planes > 1 ? 1 : spp;
    g.seg_rows = seg_rows;
    g.seg_cols = seg_cols;
    g.segs_across = segs_across;
    g.segs_down = (int)((h + seg_rows - 1) / seg_rows);
    g.planes = planes;
    g.from_decoded = from_decoded;
    g.swap = swap;
    g.row_bytes = (int64_t)seg_cols * g.sps * item;
    HYPEL_REQUIRE((int64_t)segs_across == (w + seg_cols - 1) / seg_cols, "hypel_tiff_assemble");
    HYPEL_REQUIRE((int64_t)n_segs == (int64_t)planes * segs_across * g.segs_down, "hypel_tiff_assemble");
    HYPEL_REQUIRE((int64_t)seg_cols * g.sps < (1ll << 31), "hypel_tiff_assemble");
    HYPEL_REQUIRE((int64_t)seg_rows <= (1ll << 62) / g.row_bytes, "hypel_tiff_assemble");
    const int64_t n_rows = (int64_t)n_segs * seg_rows;
    const AssemblePlan plan = plan_assemble(g, n_rows, predictor);
    HYPEL_REQUIRE(plan.blocks < (1ll << 31), "hypel_tiff_assemble");
    const hipStream_t st = ST;
    switch (item * 4 + predictor) {
        case 1 * 4 + 1: launch_assemble<1, 1>(src, segs, g, n_rows, plan, out, st); break;
        case 1 * 4 + 2: launch_assemble<1, 2>(src, segs, g, n_rows, plan, out, st); break;
        case 2 * 4 + 1: launch_assemble<2, 1>(src, segs, g, n_rows, plan, out, st); break;
        case 2 * 4 + 2: launch_assemble<2, 2>(src, segs, g, n_rows, plan, out, st); break;
        case 4 * 4 + 1: launch_assemble<4, 1>(src, segs, g, n_rows, plan, out, st); break;
        case 4 * 4 + 2: launch_assemble<4, 2>(src, segs, g, n_rows, plan, out, st); break;
        default: launch_assemble<4, 3>(src, segs, g, n_rows, plan, out, st); break;
    }
    HYPEL_CHECK_LAUNCH("hypel_tiff_assemble");
    return 0;
}
