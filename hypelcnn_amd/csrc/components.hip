// Shadow regions of a target image, relabelled where the image lives (utilities/reveal_shadow_targets.py): from "the
// mask is in HBM" to "every 8-connected region carries the class most of its lit neighbours have".
//   * components_label    : root[p] = row-major index of the first pixel of p's 8-connected component
//   * components_compact  : comp[p] = rank of that root among all roots in row-major order, and the component count
//   * components_votes    : per component, the classes of the lit pixels that touch it, its size and the winning class
//   * components_relabel  : the target image with every component that has a winner painted in that class
//   * shadow_correct      : c + c * (m * (r[b] - 1)) of a strided raster, every step rounded on its own
// Labelling is union-find over pixel indices in which a root is always the smallest index of its tree, so the result
// is the same whatever order the unions happen in.  Three launches: a tile of 64 x 16 pixels is labelled in LDS; the
// links that cross a tile border are added in a second launch, in which a parent entry is only ever touched by
// device-scope atomics (another block, possibly on another XCD, may be lowering the same entry); a third launch walks
// every pixel to its root.  No block waits for another one: a union that loses a race continues from what the atomic
// returned.  Every walk is bounded by a step cap derived from h * w; running into it sets *status and gives up.
#include "compact.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int THREADS = 256;
constexpr int TW = 64, TH = 16;             // a labelling tile
constexpr int PER = TW * TH / THREADS;      // pixels of one thread in it
constexpr int BORDER = TW + 2 * (TH - 1);   // pixels of a tile with a link that leaves it: first row, side columns
constexpr int BORDER_THREADS = 128;
static_assert(TW * TH % THREADS == 0, "a labelling tile is a whole number of block-wide strips");

// ------------------------------------------------------------------------------------------------ union-find
// LDS flavour: the tile's own table, workgroup-scope atomics.  A chain only ever descends, so TW * TH steps reach a
// root; a retry happens only when another thread lowered the same entry, which the same bound covers generously.
__device__ __forceinline__ int find_lds(const int* lab, int x) {
    for (int s = 0; s < TW * TH; ++s) {
        const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) break;
        x = p;
    }
    return x;
}

__device__ __forceinline__ bool union_lds(int* lab, int a, int b) {
    for (int s = 0; s < 4 * TW * TH; ++s) {
        a = find_lds(lab, a);
        b = find_lds(lab, b);
        if (a == b) return true;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(lab + a, b);  // hang the larger root under the smaller one
        if (old == a) return true;              // it was a root: done
        a = old;                                // somebody re-hung it meanwhile: join what it pointed to instead
    }
    return false;
}

__device__ __forceinline__ int load_parent(const int32_t* parent, int64_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// global flavour, merge launch: device-scope atomics only.  -1: the step cap ran out.
__device__ __forceinline__ int find_global(const int32_t* parent, int x, int64_t* steps) {
    for (;;) {
        const int p = load_parent(parent, x);
        if (p == x) return x;
        x = p;
        if (--*steps < 0) return -1;
    }
}

__device__ __forceinline__ bool union_global(int32_t* parent, int a, int b, int64_t cap) {
    int64_t steps = cap;
    for (;;) {
        a = find_global(parent, a, &steps);
        if (a < 0) return false;
        b = find_global(parent, b, &steps);
        if (b < 0) return false;
        if (a == b) return true;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);
        if (old == a) return true;
        a = old;
        if (--steps < 0) return false;
    }
}

// The links of pixel (x, y) to the pixels before it in scan order.  With the pixel above set, that one link is
// enough: W, NW and NE all touch it and are linked to it by their own or its turn.  Otherwise W, NW and NE each.
// visit(dx, dy) is called for every link to make.
template <typename F>
__device__ __forceinline__ void backward_links(const uint8_t* __restrict__ mask, int64_t w, int64_t x, int64_t y,
                                               F visit) {
    if (y > 0 && mask[(y - 1) * w + x] != 0) {
        visit(0, -1);
        return;
    }
    if (x > 0 && mask[y * w + x - 1] != 0) visit(-1, 0);
    if (y > 0 && x > 0 && mask[(y - 1) * w + x - 1] != 0) visit(-1, -1);
    if (y > 0 && x + 1 < w && mask[(y - 1) * w + x + 1] != 0) visit(1, -1);
}

// ------------------------------------------------------------------------------------------------ labelling
// grid (tiles across, tiles down).  parent[p] = the first pixel of p's component WITHIN the tile, -1 outside the mask.
__global__ void __launch_bounds__(THREADS) label_tile_kernel(const uint8_t* __restrict__ mask, int64_t h, int64_t w,
                                                             int32_t* __restrict__ parent,
                                                             int32_t* __restrict__ status) {
    __shared__ int lab[TW * TH];
    const int64_t x0 = (int64_t)blockIdx.x * TW, y0 = (int64_t)blockIdx.y * TH;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = k * THREADS + (int)threadIdx.x;
        const int64_t x = x0 + i % TW, y = y0 + i / TW;
        lab[i] = x < w && y < h && mask[y * w + x] != 0 ? i : -1;
    }
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = k * THREADS + (int)threadIdx.x;
        if (lab[i] < 0) continue;  // (the sign of an entry never changes)
        const int lx = i % TW, ly = i / TW;
        backward_links(mask, w, x0 + lx, y0 + ly, [&](int dx, int dy) {
            const int qx = lx + dx, qy = ly + dy;
            if (qx >= 0 && qx < TW && qy >= 0) ok &= union_lds(lab, i, qy * TW + qx);
        });
    }
    __syncthreads();
    int root[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = k * THREADS + (int)threadIdx.x;
        root[k] = lab[i] < 0 ? -1 : find_lds(lab, i);
        if (root[k] >= 0 && lab[root[k]] != root[k]) ok = false;  // find_lds ran out of steps
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = k * THREADS + (int)threadIdx.x;
        const int64_t x = x0 + i % TW, y = y0 + i / TW;
        if (x < w && y < h)
            parent[y * w + x] = root[k] < 0 ? -1 : (int32_t)((y0 + root[k] / TW) * w + x0 + root[k] % TW);
    }
    if (!ok) atomicOr(status, HYPEL_COMPONENTS_STEP_CAP);
}

// Same grid.  Only the pixels of a tile's first row and of its first and last column have links that leave the tile.
__global__ void __launch_bounds__(BORDER_THREADS) merge_borders_kernel(const uint8_t* __restrict__ mask, int64_t h,
                                                                       int64_t w, int32_t* parent, int64_t cap,
                                                                       int32_t* __restrict__ status) {
    const int64_t x0 = (int64_t)blockIdx.x * TW, y0 = (int64_t)blockIdx.y * TH;
    bool ok = true;
    // the border pixels of a tile, numbered: first row (TW), then first and last column of the other rows
    for (int e = threadIdx.x; e < BORDER; e += BORDER_THREADS) {
        const int lx = e < TW ? e : ((e - TW) & 1 ? TW - 1 : 0), ly = e < TW ? 0 : 1 + (e - TW) / 2;
        const int64_t x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h || mask[y * w + x] == 0) continue;
        backward_links(mask, w, x, y, [&](int dx, int dy) {
            const int qx = lx + dx, qy = ly + dy;
            if (qx < 0 || qx >= TW || qy < 0)
                ok &= union_global(parent, (int)(y * w + x), (int)((y + dy) * w + x + dx), cap);
        });
    }
    if (!ok) atomicOr(status, HYPEL_COMPONENTS_STEP_CAP);
}

// parent is final (a launch boundary lies behind the merge): plain loads.  Indices descend, so n steps reach a root.
__global__ void __launch_bounds__(THREADS) flatten_kernel(const int32_t* __restrict__ parent, int64_t n,
                                                          int32_t* __restrict__ root, int32_t* __restrict__ status) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        int x = parent[i];
        if (x >= 0) {
            int64_t steps = n;
            for (int p = parent[x]; p != x; p = parent[x]) {
                x = p;
                if (--steps < 0) {
                    atomicOr(status, HYPEL_COMPONENTS_STEP_CAP);
                    break;
                }
            }
        }
        root[i] = x;
    }
}

// ------------------------------------------------------------------------------------------------ compaction
// compact.h with "p is its own root" as the predicate.  comp[p] = rank for a root, -1 outside the mask; the other
// pixels are written by spread_rank_kernel, which reads only the entries of roots -- those the rank launch wrote.
struct IsRoot {
    const int32_t* __restrict__ root;
    __device__ __forceinline__ bool operator()(int64_t p) const { return root[p] == (int32_t)p; }
};

struct RootRank {
    const int32_t* __restrict__ root;
    int32_t* __restrict__ comp;
    __device__ __forceinline__ void operator()(int64_t p, int rank) const { comp[p] = rank; }
    __device__ __forceinline__ void miss(int64_t p) const {
        if (root[p] < 0) comp[p] = -1;
    }
};

__global__ void __launch_bounds__(THREADS) spread_rank_kernel(const int32_t* __restrict__ root, int64_t n,
                                                              int32_t* comp) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int r = root[i];
        if (r >= 0 && r != i) comp[i] = comp[r];
    }
}

// ------------------------------------------------------------------------------------------------ votes
// One thread per pixel.  Integer atomics only: the sums do not depend on the order they arrive in.
__global__ void __launch_bounds__(THREADS) vote_kernel(const uint8_t* __restrict__ targets,
                                                       const int32_t* __restrict__ comp, int64_t h, int64_t w,
                                                       int32_t n_components, int32_t n_classes, uint64_t exclude,
                                                       int32_t* __restrict__ votes, int32_t* __restrict__ size) {
    const int64_t n = h * w;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int c = comp[i];
        if (c < 0 || c >= n_components) continue;  // (an id past the tables: not this call's comp)
        atomicAdd(size + c, 1);
        const int64_t y = i / w, x = i - y * w;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int64_t qy = y + dy, qx = x + dx;
                if ((dy == 0 && dx == 0) || qy < 0 || qy >= h || qx < 0 || qx >= w) continue;
                const int64_t q = qy * w + qx;
                if (comp[q] >= 0) continue;
                const int t = targets[q];
                if (t < n_classes && !((exclude >> t) & 1ull)) atomicAdd(votes + (int64_t)c * n_classes + t, 1);
            }
    }
}

__global__ void __launch_bounds__(THREADS) winner_kernel(const int32_t* __restrict__ votes, int32_t n,
                                                         int32_t n_classes, uint8_t* __restrict__ winner) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    int best = 255, most = 0;
    for (int t = 0; t < n_classes; ++t) {
        const int v = votes[(int64_t)c * n_classes + t];
        if (v > most) {  // strictly more: a tie stays with the smaller class
            most = v;
            best = t;
        }
    }
    winner[c] = (uint8_t)best;
}

// ------------------------------------------------------------------------------------------------ relabel
__global__ void __launch_bounds__(THREADS) relabel_kernel(const uint8_t* __restrict__ targets,
                                                          const int32_t* __restrict__ comp,
                                                          const uint8_t* __restrict__ winner, int64_t n,
                                                          int32_t plus_one, uint8_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        int v = targets[i];
        const int c = comp[i];
        if (c >= 0) {
            const int win = winner[c];
            if (win != 255) v = win;
        }
        if (plus_one && v != 255) v += 1;
        out[i] = (uint8_t)v;
    }
}

// ------------------------------------------------------------------------------------------------ correction
// NumPy's float32 casi + casi * (map * (ratio - 1)): two products and a sum, each rounded on its own
__device__ __forceinline__ float corrected(float c, float m, float r_minus_1) {
#pragma clang fp contract(off)
    const float coef = m * r_minus_1;
    const float add = c * coef;
    return c + add;
}

template <typename T>
__global__ void __launch_bounds__(THREADS) shadow_correct_kernel(const T* __restrict__ src, int64_t h, int64_t w,
                                                                 int32_t bands, int64_t sy, int64_t sx, int64_t sb,
                                                                 const uint8_t* __restrict__ map,
                                                                 const float* __restrict__ r_minus_1,
                                                                 float* __restrict__ out) {
    const int64_t total = h * w * bands;
    for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * THREADS) {
        const int64_t pix = e / bands, y = pix / w, x = pix - y * w;
        const int b = (int)(e - pix * bands);
        const float c = (float)src[y * sy + x * sx + b * sb];
        out[e] = corrected(c, map[pix] != 0 ? 1.0f : 0.0f, r_minus_1[b]);
    }
}

template <typename T>
void launch_correct(const void* src, int64_t h, int64_t w, int32_t bands, int64_t sy, int64_t sx, int64_t sb,
                    const uint8_t* map, const float* r_minus_1, float* out, hipStream_t st) {
    hipLaunchKernelGGL(shadow_correct_kernel<T>, dim3(hypel_grid_1d(h * w * bands, THREADS)), dim3(THREADS), 0, st,
                       (const T*)src, h, w, bands, sy, sx, sb, map, r_minus_1, out);
}

bool image_ok(int64_t h, int64_t w) {
    return h > 0 && w > 0 && h < (1ll << 31) && w < (1ll << 31) && h * w < (1ll << 31);
}

}  // namespace

extern "C" int hypel_components_label_u8(const uint8_t* mask, int64_t h, int64_t w, int32_t* root, int32_t* ws,
                                         int32_t* status, hypel_stream_t stream) {
    HYPEL_REQUIRE(mask && root && ws && status && root != ws, "hypel_components_label_u8");
    HYPEL_REQUIRE(image_ok(h, w), "hypel_components_label_u8");
    const int64_t n = h * w, tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
    HYPEL_REQUIRE(tiles_y <= 65535, "hypel_components_label_u8");
    if (hipMemsetAsync(status, 0, sizeof(int32_t), ST) != hipSuccess) {
        hypel_set_error("hypel_components_label_u8: clearing the status word failed");
        return -2;
    }
    const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y);
    hipLaunchKernelGGL(label_tile_kernel, grid, dim3(THREADS), 0, ST, mask, h, w, ws, status);
    // a walk descends (at most n steps) and a retry means another union lowered an entry (at most n unions lower any)
    hipLaunchKernelGGL(merge_borders_kernel, grid, dim3(BORDER_THREADS), 0, ST, mask, h, w, ws, 4 * n + 64, status);
    hipLaunchKernelGGL(flatten_kernel, dim3(hypel_grid_1d(n, THREADS)), dim3(THREADS), 0, ST, ws, n, root, status);
    HYPEL_CHECK_LAUNCH("hypel_components_label_u8");
    return 0;
}

extern "C" int hypel_components_compact_i32(const int32_t* root, int64_t h, int64_t w, int32_t* comp,
                                            int32_t* n_components, int32_t* ws, hypel_stream_t stream) {
    HYPEL_REQUIRE(root && comp && n_components && ws && root != comp, "hypel_components_compact_i32");
    HYPEL_REQUIRE(image_ok(h, w), "hypel_components_compact_i32");
    const int64_t n = h * w;
    compact::launch(IsRoot{root}, RootRank{root, comp}, n, ws, n_components, ST);
    hipLaunchKernelGGL(spread_rank_kernel, dim3(hypel_grid_1d(n, THREADS)), dim3(THREADS), 0, ST, root, n, comp);
    HYPEL_CHECK_LAUNCH("hypel_components_compact_i32");
    return 0;
}

extern "C" int hypel_components_votes_i32(const uint8_t* targets, const int32_t* comp, int64_t h, int64_t w,
                                          int32_t n_components, int32_t n_classes, uint64_t exclude, int32_t* votes,
                                          int32_t* size, uint8_t* winner, hypel_stream_t stream) {
    HYPEL_REQUIRE(targets && comp && votes && size && winner, "hypel_components_votes_i32");
    HYPEL_REQUIRE(image_ok(h, w) && n_components >= 0 && n_components <= h * w, "hypel_components_votes_i32");
    HYPEL_REQUIRE(n_classes >= 1 && n_classes <= HYPEL_COMPONENTS_MAX_CLASSES, "hypel_components_votes_i32");
    if (n_components == 0) return 0;
    if (hipMemsetAsync(votes, 0, (size_t)n_components * n_classes * sizeof(int32_t), ST) != hipSuccess ||
        hipMemsetAsync(size, 0, (size_t)n_components * sizeof(int32_t), ST) != hipSuccess) {
        hypel_set_error("hypel_components_votes_i32: clearing the tables failed");
        return -2;
    }
    hipLaunchKernelGGL(vote_kernel, dim3(hypel_grid_1d(h * w, THREADS)), dim3(THREADS), 0, ST, targets, comp, h, w,
                       n_components, n_classes, exclude, votes, size);
    hipLaunchKernelGGL(winner_kernel, dim3((unsigned)((n_components + THREADS - 1) / THREADS)), dim3(THREADS), 0, ST,
                       votes, n_components, n_classes, winner);
    HYPEL_CHECK_LAUNCH("hypel_components_votes_i32");
    return 0;
}

extern "C" int hypel_components_relabel_u8(const uint8_t* targets, const int32_t* comp, const uint8_t* winner,
                                           int64_t h, int64_t w, int32_t plus_one, uint8_t* out,
                                           hypel_stream_t stream) {
    HYPEL_REQUIRE(targets && comp && winner && out, "hypel_components_relabel_u8");
    HYPEL_REQUIRE(image_ok(h, w), "hypel_components_relabel_u8");
    hipLaunchKernelGGL(relabel_kernel, dim3(hypel_grid_1d(h * w, THREADS)), dim3(THREADS), 0, ST, targets, comp, winner,
                       h * w, plus_one, out);
    HYPEL_CHECK_LAUNCH("hypel_components_relabel_u8");
    return 0;
}

extern "C" int hypel_shadow_correct_f32(const void* src, int32_t dtype, int64_t h, int64_t w, int32_t bands, int64_t sy,
                                        int64_t sx, int64_t sb, const uint8_t* map, const float* r_minus_1, float* out,
                                        hypel_stream_t stream) {
    HYPEL_REQUIRE(src && map && r_minus_1 && out && src != (const void*)out, "hypel_shadow_correct_f32");
    HYPEL_REQUIRE(image_ok(h, w) && bands > 0 && sy >= 0 && sx >= 0 && sb >= 0, "hypel_shadow_correct_f32");
    switch (dtype) {
        case HYPEL_DTYPE_F32: launch_correct<float>(src, h, w, bands, sy, sx, sb, map, r_minus_1, out, ST); break;
        case HYPEL_DTYPE_U16: launch_correct<uint16_t>(src, h, w, bands, sy, sx, sb, map, r_minus_1, out, ST); break;
        case HYPEL_DTYPE_I16: launch_correct<int16_t>(src, h, w, bands, sy, sx, sb, map, r_minus_1, out, ST); break;
        case HYPEL_DTYPE_U8: launch_correct<uint8_t>(src, h, w, bands, sy, sx, sb, map, r_minus_1, out, ST); break;
        default: hypel_set_error("hypel_shadow_correct_f32: unsupported dtype %d", (int)dtype); return -1;
    }
    HYPEL_CHECK_LAUNCH("hypel_shadow_correct_f32");
    return 0;
}
