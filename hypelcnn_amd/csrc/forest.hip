// Random forest of histogram trees, grown and served on the device (include/hypel.h, hypel_forest_*;
// hypelcnn_amd/classic/forest.py).
//
//   * bin_edges_kernel   : one workgroup per feature column.  The sampled rows of the column are sorted in LDS (bitonic,
//                          at most HYPEL_FOREST_EDGE_ROWS values), the quantile ranks are read off, duplicates collapse.
//   * bin_u8_kernel      : bin(x) = the number of edges < x, feature-major uint8.
//   * split_hist_kernel  : one workgroup per (active node, candidate slot): hist[bin][class] += weight with LDS integer
//                          atomics, a prefix sum over the bins per class, one score per bin boundary, the best boundary.
//   * split_apply_kernel : one workgroup per active node: the best slot, the node record, the stable partition of the
//                          node's segment of the order array (from one buffer into the other).
//   * columns_kernel     : the feature-major float32 copy of the rows (x + 0.0f), 64 x 64 tiles through LDS.
//   * split_random_kernel: extra-trees: one WAVEFRONT per (active node, candidate slot): the range of the node's raw
//                          values, one cut inside it, the class weights on either side (a per-wave LDS table, integer
//                          atomics), one score.  No block barrier: late levels are thousands of records of 2-20 rows.
//   * split_apply_kernel is one body for both searches; the side test (bin <= thr_bin, or xt <= threshold) is a functor.
//   * level_compact_kernel: one workgroup: a prefix sum over the nodes that split gives the children their node numbers
//                          and their places in the next level's active list, in active-node order.
//   * predict_kernel     : one row (or one scene pixel) per lane, one wavefront per block: the walk diverges per lane,
//                          so a block holds no second wavefront that would wait on the slowest; a node is one
//                          16-byte record, so a step is two dependent loads (the node, the value); the class sums
//                          are fp64 in LDS, one column per lane, sized by n_classes so that LDS does not cap the
//                          wavefronts per CU that hide those loads.  Which trees vote is a functor of the one
//                          walk_and_vote: all of them when serving.
//   * oob_rows_kernel    : the same walk and vote by the trees whose bootstrap left the row out; the number of votes
//                          and the means are written beside the label.
//   * permuted_hits_kernel: the same walk per (group of columns, repeat, row) with the group's columns read from a
//                          partner row; the rows still classified as y are counted by a wave sum and one integer
//                          atomic per block.
//   * importance_raw_kernel: one workgroup per (tree, window of columns): per-column fp64 sums of the nodes' impurity
//                          decreases in LDS, in node order by claiming columns (integer atomicMin), no fp atomic;
//                          normalise_rows_kernel and importance_mean_kernel finish scikit-learn's arithmetic.
// Integer atomics only (sums of int32 weights are exact and commute); every choice among equals is a total order
// (score, then feature index, then bin) and every list is built by a prefix sum, so two runs write identical bytes.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "wave.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int MAXE = HYPEL_FOREST_MAX_EDGES;
constexpr int MAXC = HYPEL_FOREST_MAX_CLASSES;
constexpr int EDGE_ROWS = HYPEL_FOREST_EDGE_ROWS;
constexpr int SORT_THREADS = 1024;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

__global__ __launch_bounds__(SORT_THREADS) void bin_edges_kernel(const float* __restrict__ x, int64_t ld, int64_t n,
                                                                 int n_s, const int32_t* __restrict__ perm, int n_bins,
                                                                 float* __restrict__ edges,
                                                                 int32_t* __restrict__ n_edges) {
    __shared__ float s[EDGE_ROWS];
    const int f = blockIdx.x, tid = threadIdx.x;
    int m = 1;
    while (m < n_s) m <<= 1;
    for (int i = tid; i < m; i += SORT_THREADS) {
        float v = INFINITY;
        if (i < n_s) {
            int64_t r = perm[i];
            if (r < 0 || r >= n) r = 0;  // (a permutation of the rows by contract; never read outside x)
            v = x[r * ld + f] + 0.0f;    // -0.0 -> +0.0: equal values have equal bits, whatever the sort does with them
        }
        s[i] = v;
    }
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += SORT_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const float a = s[i], b = s[p];
                    const bool up = (i & k) == 0;
                    if (up ? a > b : a < b) {
                        s[i] = b;
                        s[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    float* e = edges + (int64_t)f * MAXE;
    if (tid == 0) {
        const float top = s[n_s - 1];
        int ne = 0;
        for (int j = 1; j < n_bins; ++j) {
            const float v = s[(int)(((int64_t)j * n_s) / n_bins)];
            if (v >= top) break;  // an edge at the column maximum sends nothing to the right
            if (ne == 0 || v != e[ne - 1]) e[ne++] = v;
        }
        n_edges[f] = ne;
        for (int j = ne; j < MAXE; ++j) e[j] = INFINITY;
    }
}

__global__ __launch_bounds__(THREADS) void bin_u8_kernel(const float* __restrict__ x, int64_t ld, int64_t n,
                                                         int64_t row_blocks, const float* __restrict__ edges,
                                                         const int32_t* __restrict__ n_edges, uint8_t* __restrict__ bins,
                                                         int64_t ldn) {
    __shared__ float e[MAXE + 1];
    const int64_t f = blockIdx.x / row_blocks, rb = blockIdx.x - f * row_blocks;
    for (int j = threadIdx.x; j < MAXE; j += THREADS) e[j] = edges[f * MAXE + j];
    __syncthreads();
    const int64_t i = rb * THREADS + threadIdx.x;
    if (i >= n) return;
    const float v = x[i * ld + f];
    int lo = 0, hi = min(max(n_edges[f], 0), MAXE);  // the first edge >= v = the number of edges < v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    bins[f * ldn + i] = (uint8_t)lo;
}

// (valid, score descending, feature ascending, bin ascending): a total order, so any reduction tree picks the same one
struct Pick {
    double score;
    int feature, bin, valid;
};

__device__ __forceinline__ bool better(const Pick& a, const Pick& b) {
    if (a.valid != b.valid) return a.valid > b.valid;
    if (a.score != b.score) return a.score > b.score;
    if (a.feature != b.feature) return a.feature < b.feature;
    return a.bin < b.bin;
}

__device__ __forceinline__ Pick block_best(Pick p, Pick* red) {
    red[threadIdx.x] = p;
    __syncthreads();
    for (int d = THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d && better(red[threadIdx.x + d], red[threadIdx.x])) red[threadIdx.x] = red[threadIdx.x + d];
        __syncthreads();
    }
    const Pick out = red[0];
    __syncthreads();
    return out;
}

__device__ __forceinline__ double boundary_score(int64_t sl, int nl, int64_t sr, int nr) {
#pragma clang fp contract(off)
    const double a = (double)sl / (double)nl;
    const double b = (double)sr / (double)nr;
    return a + b;
}

__global__ __launch_bounds__(THREADS) void split_hist_kernel(const uint8_t* __restrict__ bins, int64_t ldn,
                                                             const int32_t* __restrict__ y,
                                                             const int32_t* __restrict__ weight, int64_t n, int C,
                                                             const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ active,
                                                             const int32_t* __restrict__ cand, int mf,
                                                             double* __restrict__ score, int32_t* __restrict__ best_bin,
                                                             int32_t* __restrict__ valid) {
    __shared__ int hist[(MAXE + 1) * MAXC];
    __shared__ Pick red[THREADS];
    const int tid = threadIdx.x;
    const int64_t a = blockIdx.x / mf;
    const int tree = active[4 * a], start = active[4 * a + 1], count = active[4 * a + 2];
    const int f = cand[blockIdx.x];
    if (count < 2) {  // (uniform over the block) one unique sample: a leaf
        if (tid == 0) {
            score[blockIdx.x] = 0.0;
            best_bin[blockIdx.x] = -1;
            valid[blockIdx.x] = 0;
        }
        return;
    }
    for (int i = tid; i < (MAXE + 1) * C; i += THREADS) hist[i] = 0;
    __syncthreads();
    const uint8_t* bf = bins + (int64_t)f * ldn;
    const int32_t* wt = weight + (int64_t)tree * n;
    for (int i = tid; i < count; i += THREADS) {
        const int s = order[start + i];
        atomicAdd(&hist[(int)bf[s] * C + y[s]], wt[s]);
    }
    __syncthreads();
    if (tid < C) {  // inclusive prefix over the bins, one class per lane
        int acc = 0;
        for (int b = 0; b <= MAXE; ++b) {
            acc += hist[b * C + tid];
            hist[b * C + tid] = acc;
        }
    }
    __syncthreads();
    Pick p = {0.0, f, tid, 0};
    if (tid < MAXE) {  // boundary tid: bins <= tid go left
        int64_t sl = 0, sr = 0;
        int nl = 0, nr = 0;
        for (int k = 0; k < C; ++k) {
            const int l = hist[tid * C + k], r = hist[MAXE * C + k] - l;
            nl += l;
            nr += r;
            sl += (int64_t)l * l;
            sr += (int64_t)r * r;
        }
        if (nl > 0 && nr > 0) {
            p.score = boundary_score(sl, nl, sr, nr);
            p.valid = 1;
        }
    }
    p = block_best(p, red);
    if (tid == 0) {
        score[blockIdx.x] = p.valid ? p.score : 0.0;
        best_bin[blockIdx.x] = p.valid ? p.bin : -1;
        valid[blockIdx.x] = p.valid;
    }
}

constexpr int TILE = 64;

// xt[c][i] = x[i][c] + 0.0f: a 64 x 64 tile read along the rows' columns and written along the columns' rows, the
// LDS tile padded by one word so that neither side meets a bank twice
__global__ __launch_bounds__(THREADS) void columns_kernel(const float* __restrict__ x, int64_t ld, int64_t n, int f,
                                                          int64_t col_tiles, float* __restrict__ xt, int64_t ldn) {
    __shared__ float tile[TILE][TILE + 1];
    const int64_t rt = blockIdx.x / col_tiles, ct = blockIdx.x - rt * col_tiles;
    const int64_t i0 = rt * TILE, c0 = ct * TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < TILE; r += WAVES)
        if (i0 + r < n && c0 + lane < f) tile[r][lane] = x[(i0 + r) * ld + c0 + lane] + 0.0f;
    __syncthreads();
    for (int c = wave; c < TILE; c += WAVES)
        if (c0 + c < f && i0 + lane < n) xt[(c0 + c) * ldn + i0 + lane] = tile[lane][c];
}

struct WaveMin {
    __device__ __forceinline__ float operator()(float a, float b) const { return b < a ? b : a; }
};
struct WaveMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return b > a ? b : a; }
};

// lo + u * (hi - lo) in float32, one rounding per operation; a cut that is not below hi (u close to 1, or hi - lo = inf)
// falls back to lo
__device__ __forceinline__ float random_cut(float lo, float hi, float u) {
#pragma clang fp contract(off)
    const float d = hi - lo;
    const float m = u * d;
    float t = lo + m;
    if (!(t < hi)) t = lo;
    return t;
}

// One wavefront per record; the block's WAVES wavefronts share nothing but the launch.  side[0 .. C) is the class
// weight left of the cut, side[MAXC .. MAXC + C) the node's: integer LDS atomics of this wavefront alone, ordered
// against its own reads by wave barriers.
__global__ __launch_bounds__(THREADS) void split_random_kernel(const float* __restrict__ xt, int64_t ldn,
                                                               const int32_t* __restrict__ y,
                                                               const int32_t* __restrict__ weight, int64_t n, int C,
                                                               const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ active,
                                                               const int32_t* __restrict__ cand,
                                                               const float* __restrict__ u, int mf, int64_t n_records,
                                                               double* __restrict__ score, float* __restrict__ thr,
                                                               int32_t* __restrict__ valid) {
    __shared__ int side_s[WAVES][2 * MAXC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rec = (int64_t)blockIdx.x * WAVES + wave;
    if (rec >= n_records) return;  // (no block barrier below)
    const int64_t a = rec / mf;
    const int tree = active[4 * a], start = active[4 * a + 1], count = active[4 * a + 2];
    const float* col = xt + (int64_t)cand[rec] * ldn;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = lane; i < count; i += 64) {
        const float v = col[order[start + i]];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    lo = wave_reduce_all(lo, WaveMin());
    hi = wave_reduce_all(hi, WaveMax());
    if (count < 2 || !(lo < hi)) {  // (uniform over the wavefront)
        if (lane == 0) {
            score[rec] = 0.0;
            thr[rec] = 0.0f;
            valid[rec] = 0;
        }
        return;
    }
    const float t = random_cut(lo, hi, u[rec]);
    int* side = side_s[wave];
    side[lane] = 0;  // 2 * MAXC == 64
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int32_t* wt = weight + (int64_t)tree * n;
    for (int i = lane; i < count; i += 64) {
        const int s = order[start + i];
        const int w = wt[s], k = y[s];
        atomicAdd(&side[MAXC + k], w);
        if (col[s] <= t) atomicAdd(&side[k], w);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int l = lane < C ? side[lane] : 0, r = lane < C ? side[MAXC + lane] - l : 0;
    const int nl = wave_sum(l), nr = wave_sum(r);
    const long long sl = wave_sum((long long)l * l), sr = wave_sum((long long)r * r);
    if (lane == 0) {
        score[rec] = boundary_score(sl, nl, sr, nr);
        thr[rec] = t;
        valid[rec] = 1;
    }
}
static_assert(2 * MAXC == 64, "split_random_kernel zeroes its table with one store per lane");

struct NodeOut {
    int32_t *feature, *thr_bin, *left, *right, *node_tree, *node_count, *node_weight;
    float* threshold;
    double* value;
};

// Which rows of a split node go left.  slot_aux(record) is the Pick's third key (the bin; the slot where the cut is a
// float: a node's columns are distinct, so it never decides); choose(pick) binds the winning slot before threshold(),
// thr_bin() and left(row) are asked.
struct BinSide {
    const uint8_t* bins;
    int64_t ldn;
    const int32_t* best_bin;
    const float* edges;
    const uint8_t* col;
    int feature, bin;
    __device__ __forceinline__ int slot_aux(int64_t at, int) const { return best_bin[at]; }
    __device__ __forceinline__ void choose(const Pick& p, int64_t) {
        col = bins + (int64_t)p.feature * ldn;
        feature = p.feature;
        bin = p.bin;
    }
    __device__ __forceinline__ float threshold() const { return edges[(int64_t)feature * MAXE + bin]; }
    __device__ __forceinline__ int thr_bin() const { return bin; }
    __device__ __forceinline__ bool left(int row) const { return (int)col[row] <= bin; }
};

struct ThrSide {
    const float* xt;
    int64_t ldn;
    const float* thr;
    const float* col;
    float t;
    __device__ __forceinline__ int slot_aux(int64_t, int slot) const { return slot; }
    __device__ __forceinline__ void choose(const Pick& p, int64_t first) {
        col = xt + (int64_t)p.feature * ldn;
        t = thr[first + p.bin];
    }
    __device__ __forceinline__ float threshold() const { return t; }
    __device__ __forceinline__ int thr_bin() const { return -1; }
    __device__ __forceinline__ bool left(int row) const { return col[row] <= t; }  // the serving walk's compare
};

template <class Side>
__global__ __launch_bounds__(THREADS) void split_apply_kernel(Side side, const int32_t* __restrict__ y,
                                                              const int32_t* __restrict__ weight, int64_t n, int C,
                                                              const int32_t* __restrict__ order_in,
                                                              int32_t* __restrict__ order_out,
                                                              const int32_t* __restrict__ active,
                                                              const int32_t* __restrict__ cand, int mf,
                                                              const double* __restrict__ score,
                                                              const int32_t* __restrict__ valid, int at_cap, NodeOut o,
                                                              int32_t* __restrict__ split_ws) {
    __shared__ int cls[MAXC];
    __shared__ Pick red[THREADS];
    __shared__ int wcount[2 * WAVES];
    __shared__ int n_left_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t a = blockIdx.x;
    const int tree = active[4 * a], start = active[4 * a + 1], count = active[4 * a + 2], node = active[4 * a + 3];
    const int32_t* wt = weight + (int64_t)tree * n;
    if (tid < MAXC) cls[tid] = 0;
    if (tid == 0) n_left_s = 0;
    __syncthreads();
    for (int i = tid; i < count; i += THREADS) {
        const int s = order_in[start + i];
        atomicAdd(&cls[y[s]], wt[s]);
    }
    Pick p = {0.0, INT_MAX, INT_MAX, 0};
    for (int s = tid; s < mf; s += THREADS) {
        const int64_t at = a * mf + s;
        const Pick q = {score[at], cand[at], side.slot_aux(at, s), valid[at]};
        if (q.valid && better(q, p)) p = q;
    }
    p = block_best(p, red);  // (its barriers also publish cls)
    int nw = 0, classes_present = 0;
    for (int k = 0; k < C; ++k) {
        nw += cls[k];
        classes_present += cls[k] > 0;
    }
    const bool leaf = count < 2 || classes_present < 2 || !p.valid || at_cap;
    if (!leaf) side.choose(p, a * mf);
    if (tid == 0) {
        o.node_tree[node] = tree;
        o.node_count[node] = count;
        o.node_weight[node] = nw;
        o.feature[node] = leaf ? -1 : p.feature;
        o.thr_bin[node] = leaf ? -1 : side.thr_bin();
        o.threshold[node] = leaf ? 0.0f : side.threshold();
        o.left[node] = -1;
        o.right[node] = -1;
    }
    if (tid < C) o.value[(int64_t)node * C + tid] = (double)cls[tid] / (double)nw;
    if (leaf) {
        if (tid == 0) split_ws[a] = 0;
        return;
    }
    // stable partition of order_in[start .. start + count) by the side test into order_out at the same place
    int mine = 0;
    for (int i = tid; i < count; i += THREADS) mine += side.left(order_in[start + i]);
    mine = wave_sum(mine);
    if (lane == 0 && mine) atomicAdd(&n_left_s, mine);
    __syncthreads();
    const int n_left = n_left_s;
    int run_l = 0, run_r = 0;
    for (int base = 0; base < count; base += THREADS) {
        const int i = base + tid;
        const bool live = i < count;
        const int s = live ? order_in[start + i] : 0;
        const bool go_left = live && side.left(s);
        const unsigned long long bl = __ballot(go_left), br = __ballot(live && !go_left);
        if (lane == 0) {
            wcount[wave] = __popcll(bl);
            wcount[WAVES + wave] = __popcll(br);
        }
        __syncthreads();  // one barrier for both sides
        int before_l, before_r, all_l, all_r;
        waves_before<WAVES>(wcount, before_l, all_l);
        waves_before<WAVES>(wcount + WAVES, before_r, all_r);
        if (go_left)
            order_out[start + run_l + before_l + wave_rank(bl)] = s;
        else if (live)
            order_out[start + n_left + run_r + before_r + wave_rank(br)] = s;
        run_l += all_l;
        run_r += all_r;
        __syncthreads();
    }
    if (tid == 0) split_ws[a] = n_left;
}

__global__ __launch_bounds__(THREADS) void level_compact_kernel(const int32_t* __restrict__ active, int n_active,
                                                                const int32_t* __restrict__ split_ws, int node_base,
                                                                int node_capacity, int32_t* __restrict__ left,
                                                                int32_t* __restrict__ right,
                                                                int32_t* __restrict__ next_active,
                                                                int32_t* __restrict__ counter) {
    __shared__ int wcount[WAVES];
    __shared__ int overflow;
    const int tid = threadIdx.x;
    if (tid == 0) overflow = 0;
    int run = 0;
    for (int base = 0; base < n_active; base += THREADS) {
        const int a = base + tid;
        const int n_left = a < n_active ? split_ws[a] : 0;
        const bool sp = n_left > 0;
        int before, all;
        const int rank = block_offsets<WAVES>(sp, wcount, before, all);
        if (sp) {
            const int r = run + before + rank;
            const int tree = active[4 * a], start = active[4 * a + 1], count = active[4 * a + 2], node = active[4 * a + 3];
            const int l = node_base + 2 * r;
            if (l + 1 < node_capacity) {
                left[node] = l;
                right[node] = l + 1;
                int32_t* q = next_active + 8 * (int64_t)r;
                q[0] = tree;
                q[1] = start;
                q[2] = n_left;
                q[3] = l;
                q[4] = tree;
                q[5] = start + n_left;
                q[6] = count - n_left;
                q[7] = l + 1;
            } else {
                overflow = 1;
            }
        }
        run += all;
        __syncthreads();
    }
    if (tid == 0) counter[0] = overflow ? -1 : 2 * run;
}

struct Model {
    const int32_t* tree_off;
    const int4* nodes;  // hypel_forest_node_t: one 16-byte load per step of the walk
    const double* leaf_value;
    int n_trees, n_nodes, n_classes;
};
static_assert(sizeof(hypel_forest_node_t) == sizeof(int4), "hypel_forest_node_t is loaded as one int4");

struct RowReader {
    const float* row;
    __device__ __forceinline__ float operator()(int feature) const { return row[feature]; }
};

struct SceneReader {  // feature = 2 * (element offset from the window origin's pixel) + (1: lidar)
    const float *casi, *lidar;
    __device__ __forceinline__ float operator()(int feature) const {
        return (feature & 1) ? lidar[feature >> 1] : casi[feature >> 1];
    }
};

constexpr int PRED_LANES = 64;

// Which trees vote for a row: every tree when serving; out of bag, the trees whose bootstrap left the row out.
struct AllTrees {
    __device__ __forceinline__ bool skip(int) const { return false; }
};
struct OutOfBag {
    const int32_t* in_bag;  // the row's column of the count table: tree t's count at in_bag[t * ldw]
    int64_t ldw;
    __device__ __forceinline__ bool skip(int t) const { return in_bag[(int64_t)t * ldw] > 0; }
};

// The winner's class index; n_votes = the trees that voted (a row without a vote has means 0 and winner 0).
template <class Reader, class Trees>
__device__ __forceinline__ int walk_and_vote(const Model& m, const Reader& read, const Trees& trees, double* acc,
                                             int lane, double* __restrict__ proba, int& n_votes) {
    const int C = m.n_classes;
    for (int k = 0; k < C; ++k) acc[k * PRED_LANES + lane] = 0.0;
    int votes = 0;
    for (int t = 0; t < m.n_trees; ++t) {
        if (trees.skip(t)) continue;
        ++votes;
        int4 rec = m.nodes[m.tree_off[t]];  // (feature, threshold bits, left, right); left < 0: leaf row -1 - left
        for (int step = 0; rec.z >= 0 && step < m.n_nodes; ++step)  // (bounded: a child's index exceeds its parent's)
            rec = m.nodes[read(rec.x) <= __int_as_float(rec.y) ? rec.z : rec.w];
        if (rec.z < 0) {
            const double* row = m.leaf_value + (int64_t)(-1 - rec.z) * C;
            for (int k = 0; k < C; ++k) acc[k * PRED_LANES + lane] += row[k];
        }
    }
    n_votes = votes;
    int best = 0;
    double bv = -1.0;
    for (int k = 0; k < C; ++k) {
        const double v = votes > 0 ? acc[k * PRED_LANES + lane] / (double)votes : 0.0;
        if (proba) proba[k] = v;
        if (v > bv) {  // the first maximum
            bv = v;
            best = k;
        }
    }
    return best;
}

__global__ __launch_bounds__(PRED_LANES) void predict_rows_kernel(const float* __restrict__ x, int64_t ld, int64_t n,
                                                                  Model m, const uint8_t* __restrict__ class_labels,
                                                                  const int32_t* __restrict__ points,
                                                                  uint8_t* __restrict__ out, int64_t raster_w,
                                                                  double* __restrict__ proba) {
    extern __shared__ double acc[];  // [n_classes][PRED_LANES]
    const int64_t i = (int64_t)blockIdx.x * PRED_LANES + threadIdx.x;
    if (i >= n) return;
    const RowReader read = {x + i * ld};
    uint8_t* o = points ? out + (int64_t)points[2 * i + 1] * raster_w + points[2 * i] : out + i;
    int votes;
    const int best = walk_and_vote(m, read, AllTrees(), acc, threadIdx.x, proba ? proba + i * m.n_classes : nullptr, votes);
    *o = class_labels ? class_labels[best] : (uint8_t)best;
}

__global__ __launch_bounds__(PRED_LANES) void predict_scene_kernel(const float* __restrict__ casi,
                                                                   const float* __restrict__ lidar, int64_t wp, int cc,
                                                                   int cl, const int32_t* __restrict__ points, int64_t n,
                                                                   Model m, const uint8_t* __restrict__ class_labels,
                                                                   uint8_t* __restrict__ out, int64_t raster_w) {
    extern __shared__ double acc[];  // [n_classes][PRED_LANES]
    const int64_t i = (int64_t)blockIdx.x * PRED_LANES + threadIdx.x;
    if (i >= n) return;
    const int64_t px = points[2 * i], py = points[2 * i + 1];
    const int64_t origin = py * wp + px;
    const SceneReader read = {casi + origin * cc, lidar ? lidar + origin * cl : nullptr};
    int votes;
    const int best = walk_and_vote(m, read, AllTrees(), acc, threadIdx.x, nullptr, votes);
    out[py * raster_w + px] = class_labels ? class_labels[best] : (uint8_t)best;
}

// ---- diagnostics: out-of-bag vote, grouped permutation hits, mean decrease in impurity ----------------------------------
__global__ __launch_bounds__(PRED_LANES) void oob_rows_kernel(const float* __restrict__ x, int64_t ld, int64_t n, Model m,
                                                              const uint8_t* __restrict__ class_labels,
                                                              const int32_t* __restrict__ weight, int64_t ldw,
                                                              uint8_t* __restrict__ out, double* __restrict__ proba,
                                                              int32_t* __restrict__ votes) {
    extern __shared__ double acc[];  // [n_classes][PRED_LANES]
    const int64_t i = (int64_t)blockIdx.x * PRED_LANES + threadIdx.x;
    if (i >= n) return;
    const RowReader read = {x + i * ld};
    const OutOfBag trees = {weight + i, ldw};
    int nv;
    const int best = walk_and_vote(m, read, trees, acc, threadIdx.x, proba + i * m.n_classes, nv);
    votes[i] = nv;
    out[i] = class_labels ? class_labels[best] : (uint8_t)best;
}

struct PermutedReader {  // the columns of group g come from the partner row
    const float *row, *other;
    int group_mod, g;
    __device__ __forceinline__ float operator()(int feature) const {
        return (feature % group_mod == g ? other : row)[feature];
    }
};

// One block per (group, repeat, 64 rows); no lane leaves before the wave sum.
__global__ __launch_bounds__(PRED_LANES) void permuted_hits_kernel(const float* __restrict__ x, int64_t ld, int64_t n,
                                                                   int64_t row_blocks, Model m,
                                                                   const int32_t* __restrict__ y,
                                                                   const int32_t* __restrict__ partner, int n_repeats,
                                                                   int group_mod, int g0, int32_t* __restrict__ hits) {
    extern __shared__ double acc[];  // [n_classes][PRED_LANES]
    const int64_t rec = blockIdx.x / row_blocks, rb = blockIdx.x - rec * row_blocks;
    const int gi = (int)(rec / n_repeats), r = (int)(rec - (int64_t)gi * n_repeats);
    const int64_t i = rb * PRED_LANES + threadIdx.x;
    int hit = 0;
    if (i < n) {
        int64_t p = partner[(int64_t)r * n + i];
        if (p < 0 || p >= n) p = i;  // (a permutation of the rows by contract; never read outside x)
        const PermutedReader read = {x + i * ld, x + p * ld, group_mod, g0 + gi};
        int votes;
        hit = walk_and_vote(m, read, AllTrees(), acc, threadIdx.x, nullptr, votes) == y[i];
    }
    hit = wave_sum(hit);
    if (threadIdx.x == 0 && hit) atomicAdd(&hits[(int64_t)gi * n_repeats + r], hit);
}

constexpr int IMP_WINDOW = HYPEL_FOREST_IMPORTANCE_WINDOW;

__device__ __forceinline__ double node_impurity(const double* __restrict__ impurity, const double* __restrict__ value,
                                                int C, int node) {
#pragma clang fp contract(off)
    if (impurity) return impurity[node];
    const double* v = value + (int64_t)node * C;
    double s = 0.0;
    for (int k = 0; k < C; ++k) {
        const double q = v[k] * v[k];
        s = s + q;
    }
    return 1.0 - s;
}

__device__ __forceinline__ double impurity_decrease(double w, double i, double wl, double il, double wr, double ir) {
#pragma clang fp contract(off)
    const double a = w * i;
    const double b = wl * il;
    const double c = wr * ir;
    const double d = a - b;
    return d - c;
}

// One workgroup per (tree, window of IMP_WINDOW columns): tab[c] sums the decreases of the tree's inner nodes on column
// c in ascending node order.  The nodes come in chunks of the block, thread k holding node base + k.  Within a chunk
// the lowest thread that still holds a decrease for a column claims it (LDS atomicMin), adds, gives the column back
// and retires; the others try again -- per column the additions happen in thread = node order, in at most THREADS
// rounds per chunk (all of them on one column).  No floating-point atomic anywhere.
__global__ __launch_bounds__(THREADS) void importance_raw_kernel(const int4* __restrict__ nodes, int n_nodes,
                                                                 const int32_t* __restrict__ tree_off, int n_trees,
                                                                 const double* __restrict__ value, int C,
                                                                 const double* __restrict__ node_weight,
                                                                 const double* __restrict__ impurity, int f, int windows,
                                                                 double* __restrict__ per_tree) {
#pragma clang fp contract(off)
    __shared__ double tab[IMP_WINDOW];
    __shared__ int claim[IMP_WINDOW];
    const int tid = threadIdx.x;
    const int t = blockIdx.x / windows, c0 = (blockIdx.x - t * windows) * IMP_WINDOW;
    const int width = min(IMP_WINDOW, f - c0);
    const int first = min(max(tree_off[t], 0), n_nodes - 1);
    const int end = t + 1 < n_trees ? min(max(tree_off[t + 1], first + 1), n_nodes) : n_nodes;
    for (int c = tid; c < width; c += THREADS) {
        tab[c] = 0.0;
        claim[c] = INT_MAX;
    }
    __syncthreads();
    for (int base = first; base < end; base += THREADS) {
        const int j = base + tid;
        int pending = 0, c = 0;
        double d = 0.0;
        if (j < end) {
            const int4 rec = nodes[j];
            // (children inside the node array by contract; a record that breaks it is passed over, never followed)
            if (rec.z >= 0 && rec.w >= 0 && rec.z < n_nodes && rec.w < n_nodes && rec.x >= c0 && rec.x < c0 + width) {
                pending = 1;
                c = rec.x - c0;
                d = impurity_decrease(node_weight[j], node_impurity(impurity, value, C, j), node_weight[rec.z],
                                      node_impurity(impurity, value, C, rec.z), node_weight[rec.w],
                                      node_impurity(impurity, value, C, rec.w));
            }
        }
        do {
            if (pending) atomicMin(&claim[c], tid);
            __syncthreads();
            const bool mine = pending && claim[c] == tid;
            __syncthreads();  // every claim is read before its holder gives it back
            if (mine) {
                tab[c] = tab[c] + d;
                claim[c] = INT_MAX;
                pending = 0;
            }
        } while (__syncthreads_or(pending));
    }
    const double w0 = node_weight[first];
    for (int c = tid; c < width; c += THREADS) per_tree[(int64_t)t * f + c0 + c] = tab[c] / w0;
}

// rows[r][0 .. f) divided by its sum where that is > 0; the sum runs over the columns in ascending order from 0.0: the
// block stages THREADS values at a time, thread 0 adds them one after the other
__global__ __launch_bounds__(THREADS) void normalise_rows_kernel(double* __restrict__ rows, int f) {
#pragma clang fp contract(off)
    __shared__ double stage[THREADS];
    __shared__ double total;
    const int tid = threadIdx.x;
    double* row = rows + (int64_t)blockIdx.x * f;
    double s = 0.0;
    for (int base = 0; base < f; base += THREADS) {
        if (base + tid < f) stage[tid] = row[base + tid];
        __syncthreads();
        if (tid == 0) {
            const int m = min(THREADS, f - base);
            for (int k = 0; k < m; ++k) s = s + stage[k];
        }
        __syncthreads();
    }
    if (tid == 0) total = s;
    __syncthreads();
    const double all = total;
    if (all > 0.0)
        for (int c = tid; c < f; c += THREADS) row[c] = row[c] / all;
}

// importances[c] = (the rows of the trees with more than one node, added in tree order from 0.0) / their number
__global__ __launch_bounds__(THREADS) void importance_mean_kernel(const double* __restrict__ per_tree,
                                                                  const int32_t* __restrict__ tree_off, int n_trees,
                                                                  int n_nodes, int f, double* __restrict__ importances,
                                                                  int32_t* __restrict__ n_used) {
#pragma clang fp contract(off)
    __shared__ int wcount[WAVES];
    const int tid = threadIdx.x;
    auto size = [&](int t) { return (t + 1 < n_trees ? tree_off[t + 1] : n_nodes) - tree_off[t]; };
    int mine = 0;
    for (int t = tid; t < n_trees; t += THREADS) mine += size(t) > 1;
    mine = wave_sum(mine);
    if ((tid & 63) == 0) wcount[tid >> 6] = mine;
    __syncthreads();
    int used = 0;
    for (int k = 0; k < WAVES; ++k) used += wcount[k];
    const int c = blockIdx.x * THREADS + tid;
    if (c < f) {
        double s = 0.0;
        for (int t = 0; t < n_trees; ++t)
            if (size(t) > 1) s = s + per_tree[(int64_t)t * f + c];
        importances[c] = used > 0 ? s / (double)used : 0.0;
    }
    if (blockIdx.x == 0 && tid == 0) n_used[0] = used;
}

}  // namespace

extern "C" int hypel_forest_bin_edges_f32(const float* x, int64_t ld, int64_t n, int32_t f, const int32_t* perm,
                                          int32_t n_bins, float* edges, int32_t* n_edges, hypel_stream_t stream) {
    HYPEL_REQUIRE(x && perm && edges && n_edges, "hypel_forest_bin_edges_f32");
    HYPEL_REQUIRE(n > 0 && f > 0 && ld >= f && n_bins >= 2 && n_bins <= MAXE + 1, "hypel_forest_bin_edges_f32");
    const int n_s = (int)(n < EDGE_ROWS ? n : EDGE_ROWS);
    hipLaunchKernelGGL(bin_edges_kernel, dim3(f), dim3(SORT_THREADS), 0, ST, x, ld, n, n_s, perm, n_bins, edges, n_edges);
    HYPEL_CHECK_LAUNCH("hypel_forest_bin_edges_f32");
    return 0;
}

extern "C" int hypel_forest_bin_u8(const float* x, int64_t ld, int64_t n, int32_t f, const float* edges,
                                   const int32_t* n_edges, uint8_t* bins, int64_t ldn, hypel_stream_t stream) {
    HYPEL_REQUIRE(x && edges && n_edges && bins, "hypel_forest_bin_u8");
    HYPEL_REQUIRE(n > 0 && f > 0 && ld >= f && ldn >= n, "hypel_forest_bin_u8");
    const int64_t row_blocks = (n + THREADS - 1) / THREADS;
    HYPEL_REQUIRE(row_blocks * f < ((int64_t)1 << 31), "hypel_forest_bin_u8");
    hipLaunchKernelGGL(bin_u8_kernel, dim3((unsigned)(row_blocks * f)), dim3(THREADS), 0, ST, x, ld, n, row_blocks, edges,
                       n_edges, bins, ldn);
    HYPEL_CHECK_LAUNCH("hypel_forest_bin_u8");
    return 0;
}

// the checks the four growth entry points share (a record is an (active node, candidate slot) pair)
static int forest_growth_args(const char* name, int64_t n, int64_t ldn, int32_t n_active, int32_t f, int32_t n_classes,
                              int32_t max_features) {
    HYPEL_REQUIRE(n > 0 && ldn >= n && n < ((int64_t)1 << 31) && n_active > 0 && f > 0, name);
    HYPEL_REQUIRE(n_classes >= 1 && n_classes <= MAXC, name);
    HYPEL_REQUIRE(max_features >= 1 && max_features <= f, name);
    HYPEL_REQUIRE((int64_t)n_active * max_features < ((int64_t)1 << 31), name);
    return 0;
}

extern "C" int hypel_forest_split_hist(const uint8_t* bins, int64_t ldn, const int32_t* y, const int32_t* weight,
                                       int64_t n, int32_t n_classes, const int32_t* order, const int32_t* active,
                                       int32_t n_active, const int32_t* cand, int32_t max_features, int32_t f,
                                       double* score, int32_t* best_bin, int32_t* valid, hypel_stream_t stream) {
    HYPEL_REQUIRE(bins && y && weight && order && active && cand && score && best_bin && valid,
                  "hypel_forest_split_hist");
    if (forest_growth_args("hypel_forest_split_hist", n, ldn, n_active, f, n_classes, max_features)) return -1;
    hipLaunchKernelGGL(split_hist_kernel, dim3((unsigned)((int64_t)n_active * max_features)), dim3(THREADS), 0, ST, bins,
                       ldn, y, weight, n, n_classes, order, active, cand, max_features, score, best_bin, valid);
    HYPEL_CHECK_LAUNCH("hypel_forest_split_hist");
    return 0;
}

// One level's apply for either search; `side` is its side test, built and checked by the caller.
template <class Side>
static int forest_split_apply(const char* name, const Side& side, const int32_t* y, const int32_t* weight, int64_t n,
                              int64_t ldn, int32_t n_classes, const int32_t* order_in, int32_t* order_out,
                              const int32_t* active, int32_t n_active, const int32_t* cand, int32_t max_features,
                              int32_t f, const double* score, const int32_t* valid, int32_t level, int32_t max_depth,
                              int32_t node_base, int32_t node_capacity, const NodeOut& o, int32_t* split_ws,
                              int32_t* next_active, int32_t* counter, hypel_stream_t stream) {
    HYPEL_REQUIRE(y && weight && order_in && order_out && order_in != order_out && active && cand && score, name);
    HYPEL_REQUIRE(valid && o.feature && o.thr_bin && o.threshold && o.left && o.right && o.node_tree, name);
    HYPEL_REQUIRE(o.node_count && o.node_weight && o.value && split_ws && next_active && counter, name);
    if (forest_growth_args(name, n, ldn, n_active, f, n_classes, max_features)) return -1;
    HYPEL_REQUIRE(level >= 0 && max_depth >= 0 && max_depth <= HYPEL_FOREST_MAX_DEPTH, name);
    HYPEL_REQUIRE(node_base >= 0 && node_capacity >= node_base, name);
    hipLaunchKernelGGL(split_apply_kernel<Side>, dim3(n_active), dim3(THREADS), 0, ST, side, y, weight, n, n_classes,
                       order_in, order_out, active, cand, max_features, score, valid, (int)(level >= max_depth), o,
                       split_ws);
    hipLaunchKernelGGL(level_compact_kernel, dim3(1), dim3(THREADS), 0, ST, active, n_active, split_ws, node_base,
                       node_capacity, o.left, o.right, next_active, counter);
    HYPEL_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int hypel_forest_split_apply(const uint8_t* bins, int64_t ldn, const int32_t* y, const int32_t* weight,
                                        int64_t n, int32_t n_classes, const int32_t* order_in, int32_t* order_out,
                                        const int32_t* active, int32_t n_active, const int32_t* cand,
                                        int32_t max_features, int32_t f, const double* score, const int32_t* best_bin,
                                        const int32_t* valid, const float* edges, int32_t level, int32_t max_depth,
                                        int32_t node_base, int32_t node_capacity, int32_t* feature, int32_t* thr_bin,
                                        float* threshold, int32_t* left, int32_t* right, int32_t* node_tree,
                                        int32_t* node_count, int32_t* node_weight, double* value, int32_t* split_ws,
                                        int32_t* next_active, int32_t* counter, hypel_stream_t stream) {
    HYPEL_REQUIRE(bins && best_bin && edges, "hypel_forest_split_apply");
    const BinSide side = {bins, ldn, best_bin, edges, nullptr, 0, 0};
    const NodeOut o = {feature, thr_bin, left, right, node_tree, node_count, node_weight, threshold, value};
    return forest_split_apply("hypel_forest_split_apply", side, y, weight, n, ldn, n_classes, order_in, order_out, active,
                              n_active, cand, max_features, f, score, valid, level, max_depth, node_base, node_capacity,
                              o, split_ws, next_active, counter, stream);
}

extern "C" int hypel_forest_columns_f32(const float* x, int64_t ld, int64_t n, int32_t f, float* xt, int64_t ldn,
                                        hypel_stream_t stream) {
    HYPEL_REQUIRE(x && xt, "hypel_forest_columns_f32");
    HYPEL_REQUIRE(n > 0 && f > 0 && ld >= f && ldn >= n, "hypel_forest_columns_f32");
    const int64_t row_tiles = (n + TILE - 1) / TILE, col_tiles = (f + TILE - 1) / TILE;
    HYPEL_REQUIRE(row_tiles * col_tiles < ((int64_t)1 << 31), "hypel_forest_columns_f32");
    hipLaunchKernelGGL(columns_kernel, dim3((unsigned)(row_tiles * col_tiles)), dim3(THREADS), 0, ST, x, ld, n, f,
                       col_tiles, xt, ldn);
    HYPEL_CHECK_LAUNCH("hypel_forest_columns_f32");
    return 0;
}

extern "C" int hypel_forest_split_random(const float* xt, int64_t ldn, const int32_t* y, const int32_t* weight,
                                         int64_t n, int32_t n_classes, const int32_t* order, const int32_t* active,
                                         int32_t n_active, const int32_t* cand, const float* u, int32_t max_features,
                                         int32_t f, double* score, float* thr, int32_t* valid, hypel_stream_t stream) {
    HYPEL_REQUIRE(xt && y && weight && order && active && cand && u && score && thr && valid,
                  "hypel_forest_split_random");
    if (forest_growth_args("hypel_forest_split_random", n, ldn, n_active, f, n_classes, max_features)) return -1;
    const int64_t n_records = (int64_t)n_active * max_features;
    hipLaunchKernelGGL(split_random_kernel, dim3((unsigned)((n_records + WAVES - 1) / WAVES)), dim3(THREADS), 0, ST, xt,
                       ldn, y, weight, n, n_classes, order, active, cand, u, max_features, n_records, score, thr, valid);
    HYPEL_CHECK_LAUNCH("hypel_forest_split_random");
    return 0;
}

extern "C" int hypel_forest_split_apply_thr(const float* xt, int64_t ldn, const int32_t* y, const int32_t* weight,
                                            int64_t n, int32_t n_classes, const int32_t* order_in, int32_t* order_out,
                                            const int32_t* active, int32_t n_active, const int32_t* cand,
                                            int32_t max_features, int32_t f, const double* score, const float* thr,
                                            const int32_t* valid, int32_t level, int32_t max_depth, int32_t node_base,
                                            int32_t node_capacity, int32_t* feature, int32_t* thr_bin, float* threshold,
                                            int32_t* left, int32_t* right, int32_t* node_tree, int32_t* node_count,
                                            int32_t* node_weight, double* value, int32_t* split_ws, int32_t* next_active,
                                            int32_t* counter, hypel_stream_t stream) {
    HYPEL_REQUIRE(xt && thr, "hypel_forest_split_apply_thr");
    const ThrSide side = {xt, ldn, thr, nullptr, 0.0f};
    const NodeOut o = {feature, thr_bin, left, right, node_tree, node_count, node_weight, threshold, value};
    return forest_split_apply("hypel_forest_split_apply_thr", side, y, weight, n, ldn, n_classes, order_in, order_out,
                              active, n_active, cand, max_features, f, score, valid, level, max_depth, node_base,
                              node_capacity, o, split_ws, next_active, counter, stream);
}

static int forest_model(const char* name, Model* m, const int32_t* tree_off, int32_t n_trees,
                        const hypel_forest_node_t* nodes, int32_t n_nodes, const double* leaf_value, int32_t n_leaves,
                        int32_t n_classes) {
    HYPEL_REQUIRE(tree_off && nodes && leaf_value, name);
    HYPEL_REQUIRE(((uintptr_t)nodes & (sizeof(int4) - 1)) == 0, name);
    HYPEL_REQUIRE(n_trees > 0 && n_nodes >= n_trees && n_leaves > 0 && n_leaves <= n_nodes, name);
    HYPEL_REQUIRE(n_classes >= 1 && n_classes <= MAXC, name);
    *m = Model{tree_off, reinterpret_cast<const int4*>(nodes), leaf_value, n_trees, n_nodes, n_classes};
    return 0;
}

// A walking launch: the model (forest_model) and the grid (forest_walk_grid) of `per_row_block` blocks per 64 rows, one
// lane a row: the block count, refused from 2^31 on (n > 0 is the caller's check), and the LDS of the class sums.
struct Walk {
    Model m;
    int64_t row_blocks;
    unsigned blocks;
    size_t lds;
};
static int forest_walk_grid(const char* name, Walk* w, int64_t n, int64_t per_row_block) {
    w->row_blocks = (n + PRED_LANES - 1) / PRED_LANES;
    HYPEL_REQUIRE(per_row_block <= INT32_MAX / w->row_blocks && "2^31 - 1 blocks at most: launch fewer groups", name);
    w->blocks = (unsigned)(per_row_block * w->row_blocks);
    w->lds = (size_t)w->m.n_classes * PRED_LANES * sizeof(double);
    return 0;
}

extern "C" int hypel_forest_predict_rows(const float* x, int64_t ld, int64_t n, int32_t f, const int32_t* tree_off,
                                         int32_t n_trees, const hypel_forest_node_t* nodes, int32_t n_nodes,
                                         const double* leaf_value, int32_t n_leaves, int32_t n_classes,
                                         const uint8_t* class_labels, const int32_t* points, uint8_t* out,
                                         int64_t raster_w, double* proba, hypel_stream_t stream) {
    const char* name = "hypel_forest_predict_rows";
    Walk w;
    if (forest_model(name, &w.m, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes)) return -1;
    HYPEL_REQUIRE(x && out, name);
    HYPEL_REQUIRE(n > 0 && f > 0 && ld >= f && (!points || raster_w > 0), name);
    if (forest_walk_grid(name, &w, n, 1)) return -1;
    hipLaunchKernelGGL(predict_rows_kernel, dim3(w.blocks), dim3(PRED_LANES), w.lds, ST, x, ld, n, w.m, class_labels,
                       points, out, raster_w, proba);
    HYPEL_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int hypel_forest_predict_scene(const float* casi, const float* lidar, int64_t hp, int64_t wp, int32_t cc,
                                          int32_t cl, const int32_t* points, int64_t n, int32_t p,
                                          const int32_t* tree_off, int32_t n_trees,
                                          const hypel_forest_node_t* scene_nodes, int32_t n_nodes,
                                          const double* leaf_value, int32_t n_leaves, int32_t n_classes,
                                          const uint8_t* class_labels, uint8_t* out, int64_t raster_w,
                                          hypel_stream_t stream) {
    const char* name = "hypel_forest_predict_scene";
    Walk w;
    if (forest_model(name, &w.m, tree_off, n_trees, scene_nodes, n_nodes, leaf_value, n_leaves, n_classes)) return -1;
    HYPEL_REQUIRE(casi && points && out && (cl == 0 || lidar), name);
    HYPEL_REQUIRE(n > 0 && p > 0 && hp >= p && wp >= p && cc > 0 && cl >= 0 && raster_w > 0, name);
    // the largest element offset a translated feature can carry must fit the int32 it is packed into
    HYPEL_REQUIRE(((int64_t)(p - 1) * wp + p) * (cc > cl ? cc : cl) < ((int64_t)1 << 30), name);
    if (forest_walk_grid(name, &w, n, 1)) return -1;
    hipLaunchKernelGGL(predict_scene_kernel, dim3(w.blocks), dim3(PRED_LANES), w.lds, ST, casi, cl ? lidar : nullptr, wp,
                       cc, cl, points, n, w.m, class_labels, out, raster_w);
    HYPEL_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int hypel_forest_oob_rows(const float* x, int64_t ld, int64_t n, int32_t f, const int32_t* tree_off,
                                     int32_t n_trees, const hypel_forest_node_t* nodes, int32_t n_nodes,
                                     const double* leaf_value, int32_t n_leaves, int32_t n_classes,
                                     const uint8_t* class_labels, const int32_t* weight, int64_t ldw, uint8_t* out,
                                     double* proba, int32_t* votes, hypel_stream_t stream) {
    const char* name = "hypel_forest_oob_rows";
    Walk w;
    if (forest_model(name, &w.m, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes)) return -1;
    HYPEL_REQUIRE(x && weight && out && proba && votes, name);
    HYPEL_REQUIRE(n > 0 && f > 0 && ld >= f && ldw >= n, name);
    if (forest_walk_grid(name, &w, n, 1)) return -1;
    hipLaunchKernelGGL(oob_rows_kernel, dim3(w.blocks), dim3(PRED_LANES), w.lds, ST, x, ld, n, w.m, class_labels, weight,
                       ldw, out, proba, votes);
    HYPEL_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int hypel_forest_permuted_hits(const float* x, int64_t ld, int64_t n, int32_t f, const int32_t* tree_off,
                                          int32_t n_trees, const hypel_forest_node_t* nodes, int32_t n_nodes,
                                          const double* leaf_value, int32_t n_leaves, int32_t n_classes,
                                          const int32_t* y, const int32_t* partner, int32_t n_repeats,
                                          int32_t group_mod, int32_t g0, int32_t n_groups, int32_t* hits,
                                          hypel_stream_t stream) {
    const char* name = "hypel_forest_permuted_hits";
    Walk w;
    if (forest_model(name, &w.m, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes)) return -1;
    HYPEL_REQUIRE(x && y && partner && hits, name);
    HYPEL_REQUIRE(n > 0 && f > 0 && ld >= f && n_repeats >= 1, name);
    HYPEL_REQUIRE(group_mod >= 1 && g0 >= 0 && n_groups >= 1 && (int64_t)g0 + n_groups <= group_mod, name);
    if (forest_walk_grid(name, &w, n, (int64_t)n_groups * n_repeats)) return -1;
    hipLaunchKernelGGL(permuted_hits_kernel, dim3(w.blocks), dim3(PRED_LANES), w.lds, ST, x, ld, n, w.row_blocks, w.m, y,
                       partner, n_repeats, group_mod, g0, hits);
    HYPEL_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int hypel_forest_importances_f64(const hypel_forest_node_t* nodes, int32_t n_nodes, const int32_t* tree_off,
                                            int32_t n_trees, const double* value, int32_t n_classes,
                                            const double* node_weight, const double* impurity, int32_t f,
                                            double* per_tree, double* importances, int32_t* n_used,
                                            hypel_stream_t stream) {
    HYPEL_REQUIRE(nodes && tree_off && node_weight && per_tree && importances && n_used, "hypel_forest_importances_f64");
    HYPEL_REQUIRE(((uintptr_t)nodes & (sizeof(int4) - 1)) == 0, "hypel_forest_importances_f64");
    HYPEL_REQUIRE(n_trees > 0 && n_nodes >= n_trees && f > 0, "hypel_forest_importances_f64");
    HYPEL_REQUIRE(impurity || (value && n_classes >= 1 && n_classes <= MAXC), "hypel_forest_importances_f64");
    const int windows = (f + IMP_WINDOW - 1) / IMP_WINDOW;
    HYPEL_REQUIRE((int64_t)n_trees * windows < ((int64_t)1 << 31), "hypel_forest_importances_f64");
    hipLaunchKernelGGL(importance_raw_kernel, dim3((unsigned)((int64_t)n_trees * windows)), dim3(THREADS), 0, ST,
                       reinterpret_cast<const int4*>(nodes), n_nodes, tree_off, n_trees, value, n_classes, node_weight,
                       impurity, f, windows, per_tree);
    hipLaunchKernelGGL(normalise_rows_kernel, dim3(n_trees), dim3(THREADS), 0, ST, per_tree, f);
    hipLaunchKernelGGL(importance_mean_kernel, dim3((f + THREADS - 1) / THREADS), dim3(THREADS), 0, ST, per_tree, tree_off,
                       n_trees, n_nodes, f, importances, n_used);
    hipLaunchKernelGGL(normalise_rows_kernel, dim3(1), dim3(THREADS), 0, ST, importances, f);
    HYPEL_CHECK_LAUNCH("hypel_forest_importances_f64");
    return 0;
}
