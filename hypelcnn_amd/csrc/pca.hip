// Band PCA of a scene that is resident as float32 pixels (classic/decomposition.py: BandPCA).
//   * pca_band_sums : per-band sums in double -- a block per chunk of pixels, partials to a workspace, fixed-order reduce
//   * pca_scatter   : S = sum over pixels of (x - mean)(x - mean)^T -- centred at load in float32, the products on the
//                     fp32 matrix cores, one float32 accumulator per chunk of HYPEL_PCA_CHUNK pixels and no more, the
//                     chunk partials added in double, in a fixed order
//   * pca_project   : out = (x - mean) W with trailing input columns copied through -- centred at load, one fmaf chain
//                     over the bands per output, the same for every row of every block
// A VIEW is h rows of w pixels of c bands: band b of pixel (y, x) is src[y * stride_y + x * stride_x + b].  Pixel p of a
// view is (p / w, p % w).  Nothing outside the c (project: c + pass) floats of a pixel is ever read.
//
// The scatter as a matrix product: the c x c output is cut into TILE x TILE tiles, of which only those on or above the
// diagonal are computed (T = nt (nt + 1) / 2 of them).  A block owns one tile and every G-th chunk of pixels; per slab of
// SLAB pixels it stages the centred values of the tile's row bands and column bands in LDS ([pixel][band]: the pixel
// axis is K for both operands) and each of its four waves multiplies a 32 x 32 quarter with 2 x 2 16x16x4 MFMA tiles.
// The next slab is fetched into registers while the current one is multiplied.
#include "common.h"

#define ST ((hipStream_t)stream)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int CHUNK = HYPEL_PCA_CHUNK;
constexpr int MAX_BLOCKS = HYPEL_PCA_MAX_BLOCKS;
constexpr int MAX_BANDS = HYPEL_PCA_MAX_BANDS;
constexpr int TILE = HYPEL_PCA_TILE;
constexpr int SLAB = 32;                          // pixels of one staged slab
constexpr int PITCH = 80;                         // = 16 mod 64: the four K rows of a fragment fall on disjoint banks
constexpr int PER = SLAB * TILE / THREADS;        // values per thread and operand of a slab
constexpr int ACC = MAX_BANDS / 64;               // band slots of a thread of the sums kernel
static_assert(TILE == 64 && CHUNK % SLAB == 0 && PER * THREADS == SLAB * TILE && PITCH >= TILE, "slab geometry");

struct View {
    const float* p;
    int64_t w, sy, sx, n;  // n = h * w pixels
    int32_t c;
};

__device__ __forceinline__ const float* pixel_at(const View& v, int64_t p) {
    const int64_t y = p / v.w;
    return v.p + y * v.sy + (p - y * v.w) * v.sx;
}

// ------------------------------------------------------------------------------------------------------ band sums
// lanes_per_pixel = min(64, c rounded up to a power of two) lanes share a pixel, lane l of them owns bands l, l + 64, ...;
// the block's THREADS / lanes_per_pixel pixel slots walk the chunk side by side.  Block g takes chunks g, g + G, ...
__global__ void __launch_bounds__(THREADS) band_sums_kernel(View v, int32_t lanes_per_pixel, int64_t n_chunks,
                                                            double* __restrict__ partial) {
    __shared__ double slots[ACC][THREADS];
    const int tid = threadIdx.x;
    const int lane = tid % lanes_per_pixel, slot = tid / lanes_per_pixel, n_slots = THREADS / lanes_per_pixel;
    double acc[ACC];
#pragma unroll
    for (int j = 0; j < ACC; ++j) acc[j] = 0.0;
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t p0 = ch * CHUNK, p1 = min(v.n, p0 + CHUNK);
        for (int64_t p = p0 + slot; p < p1; p += n_slots) {
            const float* px = pixel_at(v, p);
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const int b = lane + 64 * j;
                if (b < v.c) acc[j] += (double)px[b];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < ACC; ++j) slots[j][tid] = acc[j];
    __syncthreads();
    for (int b = tid; b < v.c; b += THREADS) {
        double sum = 0.0;
        for (int s = 0; s < n_slots; ++s) sum += slots[b >> 6][s * lanes_per_pixel + (b & 63)];
        partial[(int64_t)blockIdx.x * v.c + b] = sum;
    }
}

__global__ void __launch_bounds__(THREADS) reduce_sums_kernel(const double* __restrict__ partial, int32_t blocks,
                                                              int32_t c, double* __restrict__ sums) {
    // a block per band: thread t adds partials t, t + THREADS, ... in that order, then a fixed halving tree
    __shared__ double part[THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    double sum = 0.0;
    for (int g = tid; g < blocks; g += THREADS) sum += partial[(int64_t)g * c + b];
    part[tid] = sum;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    if (tid == 0) sums[b] = part[0];
}

// -------------------------------------------------------------------------------------------------------- scatter
// index of tile (ti <= tj) among the nt (nt + 1) / 2 tiles on or above the diagonal, row after row
__host__ __device__ __forceinline__ int tile_index(int ti, int tj, int nt) { return ti * nt - ti * (ti - 1) / 2 + (tj - ti); }

// one thread's share of a slab: band tid % 64 of the row tile and of the column tile, pixels tid / 64 + 4 * it
struct Staged {
    float a[PER], b[PER];
};

__device__ __forceinline__ void fetch_slab(const View& v, const float* __restrict__ mean, int i0, int j0, bool diag,
                                           int64_t p0, int64_t p1, int tid, Staged& st) {
    const int col = tid & 63, sub = tid >> 6;
    const int bi = i0 + col, bj = j0 + col;
    const bool vi = bi < v.c, vj = !diag && bj < v.c;
    const float mi = vi ? mean[bi] : 0.0f, mj = vj ? mean[bj] : 0.0f;
#pragma unroll
    for (int it = 0; it < PER; ++it) {
        const int64_t p = p0 + sub + 4 * it;
        const bool vp = p < p1;
        const float* px = pixel_at(v, vp ? p : p0);
        // outside the chunk or the bands: zeros, which add nothing
        st.a[it] = (vp && vi) ? px[bi] - mi : 0.0f;
        st.b[it] = (vp && vj) ? px[bj] - mj : 0.0f;
    }
}

__device__ __forceinline__ void store_slab(const Staged& st, bool diag, int tid, float* a_s, float* b_s) {
    const int col = tid & 63, sub = tid >> 6;
#pragma unroll
    for (int it = 0; it < PER; ++it) {
        a_s[(sub + 4 * it) * PITCH + col] = st.a[it];
        if (!diag) b_s[(sub + 4 * it) * PITCH + col] = st.b[it];
    }
}

// grid (T tiles, G chunk groups); partial: [G][T][TILE][TILE] doubles
__global__ void __launch_bounds__(THREADS) scatter_kernel(View v, const float* __restrict__ mean, int32_t nt,
                                                          int64_t n_chunks, double* __restrict__ partial) {
    __shared__ float a_s[SLAB * PITCH];
    __shared__ float b_s[SLAB * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = lane & 15, k = lane >> 4;
    int ti = 0, rest = blockIdx.x;  // (uniform) the tile of this block
    while (rest >= nt - ti) {
        rest -= nt - ti;
        ++ti;
    }
    const int tj = ti + rest;
    const bool diag = ti == tj;
    const int i0 = ti * TILE, j0 = tj * TILE;
    const int wi = (wv >> 1) * 32, wj = (wv & 1) * 32;  // the wave's quarter of the tile
    const float* a_rd = a_s + k * PITCH + wi + n;
    const float* b_rd = (diag ? a_s : b_s) + k * PITCH + wj + n;
    double total[2][2][4];
#pragma unroll
    for (int q = 0; q < 16; ++q) (&total[0][0][0])[q] = 0.0;
    Staged st;
    for (int64_t ch = blockIdx.y; ch < n_chunks; ch += gridDim.y) {
        const int64_t p0 = ch * CHUNK, p1 = min(v.n, p0 + CHUNK);
        f32x4 acc[2][2];  // one chunk and no more
#pragma unroll
        for (int q = 0; q < 4; ++q) (&acc[0][0])[q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        fetch_slab(v, mean, i0, j0, diag, p0, p1, tid, st);
        for (int64_t s0 = p0; s0 < p1; s0 += SLAB) {
            __syncthreads();  // the previous slab has been read
            store_slab(st, diag, tid, a_s, b_s);
            __syncthreads();
            if (s0 + SLAB < p1) fetch_slab(v, mean, i0, j0, diag, s0 + SLAB, p1, tid, st);  // in flight meanwhile
#pragma unroll
            for (int kk = 0; kk < SLAB; kk += 4) {
                const float a0 = a_rd[kk * PITCH], a1 = a_rd[kk * PITCH + 16];
                const float b0 = b_rd[kk * PITCH], b1 = b_rd[kk * PITCH + 16];
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) total[x][y][r] += (double)acc[x][y][r];
    }
    double* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (TILE * TILE);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(wi + 16 * x + 4 * k + r) * TILE + wj + 16 * y + n] = total[x][y][r];
}

// a thread per output: the entry on or above the diagonal (of the matrix, and so of a diagonal tile) serves both halves
__global__ void __launch_bounds__(THREADS) reduce_scatter_kernel(const double* __restrict__ partial, int32_t groups,
                                                                 int32_t nt, int32_t c, double* __restrict__ scatter) {
    const int64_t id = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (id >= (int64_t)c * c) return;
    int i = (int)(id / c), j = (int)(id - (int64_t)i * c);
    if (i > j) {
        const int t = i;
        i = j;
        j = t;
    }
    const int tiles = nt * (nt + 1) / 2;
    const double* src = partial + (int64_t)tile_index(i / TILE, j / TILE, nt) * (TILE * TILE) + (i % TILE) * TILE + j % TILE;
    double sum = 0.0;
    for (int g = 0; g < groups; ++g) sum += src[(int64_t)g * tiles * (TILE * TILE)];
    scatter[id] = sum;
}

// -------------------------------------------------------------------------------------------------------- project
constexpr int PR = 64;   // rows of a block
constexpr int PB = 64;   // bands of a staged chunk
constexpr int PK = 64;   // output columns of a pass
constexpr int XP = PB + 1;  // odd: the four rows a lane group reads fall on different banks

// thread (cg = tid % 16, rg = tid / 16) owns rows rg * 4 .. + 3 and columns cg, cg + 16, cg + 32, cg + 48 of the pass.
// Every output is ONE chain acc = fmaf(x[b] - mean[b], W[b][j], acc) over b = 0 .. c - 1 from acc = 0: the order does
// not know the row, the block or the pass of the grid.
__global__ void __launch_bounds__(THREADS) project_kernel(View v, int32_t pass, const float* __restrict__ mean,
                                                          const float* __restrict__ weights, int32_t k,
                                                          float* __restrict__ out, int64_t ldo) {
    __shared__ float x_s[PR * XP];
    __shared__ float w_s[PB * PK];
    const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4;
    const int64_t n_blocks = (v.n + PR - 1) / PR;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t r0 = blk * PR;
        for (int jt = 0; jt < k; jt += PK) {
            float acc[4][4];
#pragma unroll
            for (int q = 0; q < 16; ++q) (&acc[0][0])[q] = 0.0f;
            for (int b0 = 0; b0 < v.c; b0 += PB) {
                __syncthreads();  // the previous chunk has been read
                {   // rows: thread reads band tid % 64 of rows tid / 64 + 4 * it, centred
                    const int col = tid & 63, sub = tid >> 6, b = b0 + col;
                    const bool vb = b < v.c;
                    const float m = vb ? mean[b] : 0.0f;
#pragma unroll 4
                    for (int it = 0; it < PR / 4; ++it) {
                        const int row = sub + 4 * it;
                        const int64_t r = r0 + row;
                        x_s[row * XP + col] = (vb && r < v.n) ? pixel_at(v, r)[b] - m : 0.0f;
                    }
                    // weights: column tid % 64 of bands tid / 64 + 4 * it
                    const int j = jt + col;
#pragma unroll 4
                    for (int it = 0; it < PB / 4; ++it) {
                        const int bb = b0 + sub + 4 * it;
                        w_s[(sub + 4 * it) * PK + col] = (bb < v.c && j < k) ? weights[(int64_t)bb * k + j] : 0.0f;
                    }
                }
                __syncthreads();
                const int nb = min(PB, v.c - b0);
                for (int b = 0; b < nb; ++b) {
                    float xv[4], wv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) xv[r] = x_s[(rg * 4 + r) * XP + b];
#pragma unroll
                    for (int q = 0; q < 4; ++q) wv[q] = w_s[b * PK + cg + 16 * q];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[r][q] = fmaf(xv[r], wv[q], acc[r][q]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = r0 + rg * 4 + r;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = jt + cg + 16 * q;
                    if (row < v.n && j < k) out[row * ldo + j] = acc[r][q];
                }
            }
        }
        // trailing input columns, bit for bit
        for (int e = tid; e < PR * pass; e += THREADS) {
            const int64_t row = r0 + e / pass;
            const int j = e % pass;
            if (row < v.n) out[row * ldo + k + j] = pixel_at(v, row)[v.c + j];
        }
    }
}

constexpr int64_t MAX_PIXELS = 1ll << 40, MAX_STRIDE = 1ll << 40;

// h, w >= 1, c in 1 .. HYPEL_PCA_MAX_BANDS, both strides >= c (`tail` more floats of a pixel are read: project's pass)
bool view_ok(int64_t h, int64_t w, int32_t c, int64_t sy, int64_t sx, int64_t tail) {
    return h >= 1 && w >= 1 && h <= MAX_PIXELS && w <= MAX_PIXELS && h * w <= MAX_PIXELS && c >= 1 && c <= MAX_BANDS &&
           sy >= c + tail && sx >= c + tail && sy <= MAX_STRIDE && sx <= MAX_STRIDE;
}

// floats from the first to one past the last the view reads
int64_t view_span(int64_t h, int64_t w, int32_t c, int64_t sy, int64_t sx, int64_t tail) {
    return (h - 1) * sy + (w - 1) * sx + c + tail;
}

bool apart(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + (uintptr_t)a_bytes <= y || y + (uintptr_t)b_bytes <= x;
}

int64_t chunks_of(int64_t n) { return (n + CHUNK - 1) / CHUNK; }

}  // namespace

extern "C" int hypel_pca_band_sums_f64(const float* x, int64_t h, int64_t w, int32_t c, int64_t stride_y,
                                       int64_t stride_x, double* sums, double* ws, int64_t ws_doubles,
                                       hypel_stream_t stream) {
    HYPEL_REQUIRE(x && sums && ws && sums != ws, "hypel_pca_band_sums_f64");
    HYPEL_REQUIRE(view_ok(h, w, c, stride_y, stride_x, 0), "hypel_pca_band_sums_f64");
    const int64_t n = h * w, n_chunks = chunks_of(n);
    const int64_t blocks = n_chunks < MAX_BLOCKS ? n_chunks : MAX_BLOCKS;
    HYPEL_REQUIRE(ws_doubles >= blocks * c, "hypel_pca_band_sums_f64");
    HYPEL_REQUIRE(apart(x, view_span(h, w, c, stride_y, stride_x, 0) * 4, sums, (int64_t)c * 8) &&
                      apart(x, view_span(h, w, c, stride_y, stride_x, 0) * 4, ws, blocks * c * 8) &&
                      apart(sums, (int64_t)c * 8, ws, blocks * c * 8),
                  "hypel_pca_band_sums_f64");
    int lanes = 1;
    while (lanes < c && lanes < 64) lanes *= 2;
    const View v{x, w, stride_y, stride_x, n, c};
    hipLaunchKernelGGL(band_sums_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, ST, v, lanes, n_chunks, ws);
    hipLaunchKernelGGL(reduce_sums_kernel, dim3((unsigned)c), dim3(THREADS), 0, ST, ws,
                       (int32_t)blocks, c, sums);
    HYPEL_CHECK_LAUNCH("hypel_pca_band_sums_f64");
    return 0;
}

extern "C" int hypel_pca_scatter_f64(const float* x, int64_t h, int64_t w, int32_t c, int64_t stride_y, int64_t stride_x,
                                     const float* mean, double* scatter, double* ws, int64_t ws_doubles,
                                     hypel_stream_t stream) {
    HYPEL_REQUIRE(x && mean && scatter && ws && scatter != ws, "hypel_pca_scatter_f64");
    HYPEL_REQUIRE(view_ok(h, w, c, stride_y, stride_x, 0), "hypel_pca_scatter_f64");
    const int64_t n = h * w, n_chunks = chunks_of(n);
    const int nt = (c + TILE - 1) / TILE, tiles = nt * (nt + 1) / 2;
    const int64_t room = MAX_BLOCKS / tiles;  // >= 1: at most 36 tiles
    const int64_t groups = n_chunks < room ? n_chunks : room;
    const int64_t need = groups * tiles * (TILE * TILE);
    HYPEL_REQUIRE(ws_doubles >= need, "hypel_pca_scatter_f64");
    const int64_t span = view_span(h, w, c, stride_y, stride_x, 0) * 4;
    HYPEL_REQUIRE(apart(x, span, scatter, (int64_t)c * c * 8) && apart(x, span, ws, need * 8) &&
                      apart(mean, (int64_t)c * 4, scatter, (int64_t)c * c * 8) && apart(mean, (int64_t)c * 4, ws, need * 8) &&
                      apart(scatter, (int64_t)c * c * 8, ws, need * 8),
                  "hypel_pca_scatter_f64");
    const View v{x, w, stride_y, stride_x, n, c};
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)tiles, (unsigned)groups), dim3(THREADS), 0, ST, v, mean, nt,
                       n_chunks, ws);
    hipLaunchKernelGGL(reduce_scatter_kernel, dim3((unsigned)(((int64_t)c * c + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                       ST, ws, (int32_t)groups, nt, c, scatter);
    HYPEL_CHECK_LAUNCH("hypel_pca_scatter_f64");
    return 0;
}

extern "C" int hypel_pca_project_f32(const float* x, int64_t h, int64_t w, int32_t c, int64_t stride_y, int64_t stride_x,
                                     int32_t pass, const float* mean, const float* weights, int32_t k, float* out,
                                     int64_t ldo, hypel_stream_t stream) {
    HYPEL_REQUIRE(x && mean && weights && out, "hypel_pca_project_f32");
    HYPEL_REQUIRE(pass >= 0 && pass <= MAX_BANDS, "hypel_pca_project_f32");
    HYPEL_REQUIRE(view_ok(h, w, c, stride_y, stride_x, pass), "hypel_pca_project_f32");
    HYPEL_REQUIRE(k >= 1 && k <= c, "hypel_pca_project_f32");
    HYPEL_REQUIRE(ldo >= (int64_t)k + pass && ldo <= MAX_STRIDE, "hypel_pca_project_f32");
    const int64_t n = h * w;
    const int64_t out_bytes = ((n - 1) * ldo + k + pass) * 4;
    HYPEL_REQUIRE(apart(x, view_span(h, w, c, stride_y, stride_x, pass) * 4, out, out_bytes) &&
                      apart(mean, (int64_t)c * 4, out, out_bytes) && apart(weights, (int64_t)c * k * 4, out, out_bytes),
                  "hypel_pca_project_f32");
    const View v{x, w, stride_y, stride_x, n, c};
    const int64_t n_blocks = (n + PR - 1) / PR;
    const int64_t blocks = n_blocks < HYPEL_PCA_PROJECT_MAX_BLOCKS ? n_blocks : HYPEL_PCA_PROJECT_MAX_BLOCKS;
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, ST, v, pass, mean, weights, k, out, ldo);
    HYPEL_CHECK_LAUNCH("hypel_pca_project_f32");
    return 0;
}
