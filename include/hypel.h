/* hypel.h -- C-ABI of libhypel_hip.so: the MI355X (gfx950) compute path behind the
 * NNModel / GAN-wrapper plugin API of aligokalppeker/hypelcnn.
 *
 * The reference has NO native layer: every entry point below replaces a call the reference
 * makes into TensorFlow / tf_slim kernels (reference file:line cited per function).  The
 * binding a maintainer would add on the reference side is a ctypes stub.
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer unless it says "host".
 *  - all work is enqueued asynchronously on `stream` (a hipStream_t); no implicit syncs,
 *    no allocation; the caller (PyTorch caching allocator on the Python side) owns every
 *    buffer including workspaces.
 *  - return 0 on success, negative on error; message via hypel_last_error() (thread-local).
 *  - activations are row-major matrices [rows, C] with a leading dimension `ld` (floats).
 *    Internally the host keeps patch tensors PIXEL-MAJOR: [P = H*W][N][C], i.e. the rows
 *    of pixel p for the whole minibatch are contiguous.  That turns a SAME convolution
 *    into a sum over VALID taps of plain GEMMs on contiguous row blocks (no im2col, no
 *    padding taps): see hypel_seg_gemm_f32.  hypel_nhwc_to_pnc converts the loader's
 *    NHWC batches (importer/InMemoryImporter.py:27-38).
 *  - weights keep the TF variable layouts: conv HWIO [kh][kw][Cin][Cout], FC [in][out],
 *    BN vectors [C] -- checkpoints keyed by TF names map 1:1.
 */
#ifndef HYPEL_H
#define HYPEL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hypel_stream_t; /* hipStream_t */

#define HYPEL_ABI_VERSION 8  /* bump whenever a prototype, a struct layout or the meaning of a flag changes */

/* activation codes (leaky_relu: HYPELCNNModel.py:39, DUALCNNModel.py:18, shadow_data_models.py:53;
 * relu: tf_slim default, CONCNNModel.py; sigmoid: HYPELCNNModel.py:93; tanh: shadow_data_models.py:86) */
enum { HYPEL_ACT_NONE = 0, HYPEL_ACT_LRELU = 1, HYPEL_ACT_RELU = 2, HYPEL_ACT_SIGMOID = 3, HYPEL_ACT_TANH = 4 };

int hypel_version(void);
const char* hypel_last_error(void);
/* number of compute units / XCDs of the current device (host query, for table building) */
int hypel_device_info(int32_t* n_cu, int32_t* n_xcd);

/* host helper: CRC-32C (Castagnoli) of `n` bytes continued from `crc` (0 to start); used by the TensorFlow checkpoint
 * bundle reader/writer (monitored_session_runner.py:164-171 saves, cycle_gan_wrapper.py:140-147 restores such files) */
uint32_t hypel_crc32c(uint32_t crc, const void* data, uint64_t n);

/* ---- layout ------------------------------------------------------------------------------- */
/* x[N][P][C] (NHWC with P=H*W) -> out[P][N][ld] (pad columns zeroed).  Replaces the
 * feed_dict/prefetch_to_device hand-over (InMemoryImporter.py:80-83, common_nn_ops.py:200). */
int hypel_nhwc_to_pnc(const float* x, float* out, int64_t n, int32_t p, int32_t c, int64_t ld,
                      hypel_stream_t stream);
int hypel_pnc_to_nhwc(const float* in, int64_t ld, float* x, int64_t n, int32_t p, int32_t c,
                      hypel_stream_t stream);
int hypel_fill_f32(float* dst, int64_t count, float value, hypel_stream_t stream);

/* ---- grouped multi-segment GEMM (fp32 MFMA, 32x32x2) ------------------------------------------
 * For every group g:  C_g[rows_g x n] (+)= sum_{s in segs(g)} op(A_s)[rows_g x k_s] * op(B_s)[k_s x n] (+ bias)
 *   trans_a = 0: op(A_s)[i][kk] = A[a_off + i*lda + kk]      trans_a = 1: A[a_off + kk*lda + i]
 *   trans_b = 0: op(B_s)[kk][j] = B[b_off + kk*ldb + j]      trans_b = 1: B[b_off + j*ldb + kk]
 *   C_g[i][j] = C[c_off + i*ldc + j]
 * One kernel covers: tf_slim.conv2d 1x1 and kxk SAME as exact-tap sums (HYPELCNNModel.py:136,
 * 157,177; DUALCNNModel.py:99; CONCNNModel.py:33-60), tf_slim.fully_connected incl. the
 * flatten that precedes it (HYPELCNNModel.py:74-94,121; DUALCNNModel.py:31,48-54), and their
 * data-gradient (trans_b=1) and filter-gradient (trans_a=1, split over rows) passes that
 * tf.gradients derives inside create_train_op (common_nn_ops.py:232).
 * bias (optional) is indexed by the ABSOLUTE output column, (c_off mod ldc) + j, so the branches of a
 * merged multi-kernel level (groups starting at different channel offsets) share one launch.
 * `tiles` lists every 128-row output tile: its group and first row, plus a copy of what the kernel needs to start the
 * tile (the group's rows / segment range / c_off and the first segment), so that a block reads ONE record before its
 * first operand loads instead of chasing tiles -> groups -> segs; tables live on the device. */
typedef struct { int64_t a_off; int64_t b_off; int32_t k; int32_t reserved; } hypel_seg_t;
typedef struct { int64_t c_off; int32_t seg_begin; int32_t seg_count; int32_t rows; int32_t reserved; } hypel_group_t;
typedef struct {
    int32_t group; int32_t m0;                         /* output rows [m0, min(m0 + 128, rows)) of groups[group] */
    int32_t rows; int32_t seg_begin; int32_t seg_count; /* copies of groups[group] */
    int32_t k0; int64_t c_off; int64_t a_off0; int64_t b_off0; /* c_off copy; segs[seg_begin] copy (0 if none) */
    int32_t flags; int32_t n;                          /* HYPEL_TILE_*; n > 0: THIS tile's group has n output columns (<= the launch's n) */
} hypel_tile_t;
#define HYPEL_GEMM_BM 128
/* K-slice records (round 6; tail splitting for the 512-slot split-operand kernels): the segment list of a heavy output tile
 * -- or of the last, partly filled round of a launch -- is cut into slices that run as blocks of their own.  Slice 0 is an
 * ordinary record of the launch (bias, accumulate, shortcut gather apply to it); the other slices carry HYPEL_TILE_PLAIN:
 * their block writes its partial sum to its own c_off (a scratch region, addressed relative to `c` like every c_off)
 * and IGNORES the launch's bias / accumulate bit / shortcut operands.  The caller adds the partials to the output in a
 * fixed order afterwards (hypel_reduce_splits_multi_sized_f32, accumulate flag set): deterministic, no atomics.  Not
 * valid in hypel_seg_gemm_stats_f32 launches and with HYPEL_GEMM_ACT_* (their epilogues need the whole sum). */
#define HYPEL_TILE_PLAIN 1
/* Short segments (data gradients through convolutions with <= 16 filters: K = 15 in the narrowest HYPELCNN level):
 * a segment whose `k` has HYPEL_SEG_PAIR_FLAG set (real k = k & ~flag, <= 16) shares ONE 32-column k-tile with the
 * NEXT segment of its group (k <= 16, flag clear); the tile record's k0 copy carries the flag too.  Launches whose
 * tables contain such pairs pass HYPEL_GEMM_PAIRED_SEGS in `accumulate` (trans_a = 0, trans_b = 1, n > 16 only; the
 * two a_off / b_off of a pair must be less than 2 GB apart).  Results do not depend on pairing. */
#define HYPEL_SEG_PAIR_FLAG 0x40000000
#define HYPEL_GEMM_PAIRED_SEGS 0x400
/* Hint: every group of the launch has exactly ONE segment (a 1x1 convolution or its data gradient).  With 128x32 blocks
 * such launches run on a build of the kernel that keeps 7 instead of 6 blocks resident per CU.  Results do not depend
 * on the hint. */
#define HYPEL_GEMM_SINGLE_SEG 0x800

/* Merged multi-kernel levels (nnmodel/HYPELCNNModel.py:167-183, DUALCNNModel.py:92-104).  The kernel sizes of a level
 * are nested (1 c 3 c 5 c 7 ...): an input offset at ring r = max(|dy|, |dx|) belongs to every branch with
 * k >= 2r + 1, a SUFFIX of the concat order, so its output columns are ONE contiguous range [r * cout, C).  With a
 * packed weight image W_pack[offset][Cin][C] (hypel_copy_blocks_f32 builds it from the HWIO variables) a level is, per
 * output pixel and ring, a plain product on that column range: groups of one launch then differ in their column
 * count, which travels in hypel_tile_t.n (0 = the launch's n; the grid covers the widest group, blocks beyond a
 * narrower group's columns exit).  HYPEL_GEMM_MFMA16X4 (n <= 64, trans_a = trans_b = 0): 128x64 blocks on the 16x16x4
 * MFMA, four 16-column tiles per wave, for levels with <= 16 filters per branch; HYPEL_GEMM_VAR_N: the tile records
 * carry column counts -- 128x64 blocks then skip an accumulator tile that lies outside their group.  Results depend
 * on neither (a launch without them computes the unused tiles on zeros). */
#define HYPEL_GEMM_MFMA16X4 0x2000
#define HYPEL_GEMM_VAR_N 0x4000
/* Activation in the product's epilogue (hypel_seg_gemm_f32, trans_a = trans_b = 0, no accumulate): C = lrelu(product + bias)
 * with the slope the code names -- a tf_slim.fully_connected(activation_fn=leaky_relu) WITHOUT a normaliser in one launch
 * (gan/shadow_data_models.py:95-149: the critics' and feature-discriminator layers, slope 0.1).  The slopes are a closed
 * list so that the constant is exact fp32 (no float travels in `accumulate`).  Backward passes take act' from the sign of
 * the OUTPUT, which a positive slope preserves. */
#define HYPEL_GEMM_ACT_LRELU_0_1 0x10000
#define HYPEL_GEMM_ACT_LRELU_0_18 0x20000
#define HYPEL_GEMM_ACT_LRELU_0_2 0x30000
#define HYPEL_GEMM_ACT_LRELU_0_01 0x40000
/* fp32 products on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, 16x the rate of v_mfma_f32_32x32x2_f32).  Every
 * fp32 operand element is split EXACTLY into three round-to-nearest bf16 parts (x = hi + mid + lo: 8 + 8 + 8 significand
 * bits, fp32's exponent range) on its way into LDS; each k-step issues the six partial products hi hi, hi mid, mid hi,
 * hi lo, lo hi, mid mid (every one exact in the fp32 accumulator) and drops mid lo, lo mid, lo lo, which are below
 * 2^-24 |a b| -- the rounding unit of the fp32 accumulate itself.  Inputs, outputs, tables and epilogues (bias,
 * accumulate, shortcut gather, statistics) are those of the plain launch; the result is as accurate as the fp32 MFMA
 * chain (tests/test_gpu_kernels.py::test_seg_gemm_split6_error_vs_fp32_chain measures max |c - fp64| / sum |a b| of
 * both on every launch shape of the benchmark step) but not bit-identical to it.  Plain products only (no paired
 * segments, MFMA16X4, ACT; HYPEL_GEMM_VAR_N is fine), n > 16, not trans_a = trans_b = 1.  With this flag the tile-width hint reads
 * 1 = 128x32, 2 = 128x64, 3 = 128x128 blocks.  hypel_seg_gemm_multi_f32: OR HYPEL_GEMM_MULTI_SPLIT6 into tile_width
 * (32, 64 or 128 then).
 * Limits of the claim (tests/test_gpu_kernels.py::test_seg_gemm_split6_hard_operands, ..._nonfinite_and_extreme_operands):
 *  - non-finite operands: an Inf splits into hi = Inf, mid = Inf - Inf = NaN, so a product the fp32 chain evaluates to
 *    +-Inf comes out NaN here (a NaN operand gives NaN on both paths).  Non-finite stays non-finite -- the loss guard
 *    (hypel_loss_guard, NanTensorHook's counterpart) fires either way -- but Inf is not distinguished from NaN;
 *  - finite |x| >= 2^128 - 2^119 (above bf16's largest finite value, 3.3895e38: the top 0.4 % of fp32's last binade)
 *    rounds hi to Inf and gives NaN where the fp32 chain would give a huge finite number or Inf;
 *  - |x| < 2^-110: the lo (then the mid) part is a bf16 subnormal, which the matrix cores flush to zero -- the operand
 *    keeps 16 (then 8) significand bits instead of 24; products of such operands are below fp32's own subnormal range
 *    against any operand of ordinary magnitude;
 *  - from 2^-110 up to bf16's maximum the result stays within a few 2^-24 of sum |a b| whatever the mix of signs and
 *    magnitudes in a row: cancellation does not hurt (the partial products are exact), and where ONE product dominates a
 *    row's sum (operands spanning tens of binades) its partial products enter the accumulator as three non-negligible
 *    additions instead of the chain's one -- measured 1.5 x the fp32 chain's error there (7.3e-7 vs 4.7e-7 of sum |a b|),
 *    bounded by 3 x. */
#define HYPEL_GEMM_SPLIT6 0x8000
#define HYPEL_GEMM_MULTI_SPLIT6 0x100

/* `accumulate`: bit 0 = add to C instead of overwriting it; bits 8-9 = optional tile-width hint
 * (0 = library heuristic, 1 = 128x32 blocks, 2 = 128x64 blocks, 3 = 128x96 blocks for n > 64) -- results do not
 * depend on it; bit 10 = HYPEL_GEMM_PAIRED_SEGS; bit 11 = HYPEL_GEMM_SINGLE_SEG;
 * bit 13 = HYPEL_GEMM_MFMA16X4; bit 14 = HYPEL_GEMM_VAR_N; bit 15 = HYPEL_GEMM_SPLIT6; bits 16-18 = HYPEL_GEMM_ACT_*. */
int hypel_seg_gemm_f32(const float* a, int64_t lda, int32_t trans_a, const float* b, int64_t ldb, int32_t trans_b,
                       float* c, int64_t ldc, int32_t n, const hypel_group_t* groups, const hypel_seg_t* segs,
                       const hypel_tile_t* tiles, int32_t n_tiles, const float* bias, int32_t accumulate,
                       hypel_stream_t stream);

/* hypel_seg_gemm_f32 that also leaves the batch-norm statistics of its output (tf_slim.batch_norm under the conv /
 * fully_connected arg_scope, nnmodel/HYPELCNNModel.py:37,40-45): for a launch with ONE group (a 1x1 convolution or
 * a dense layer: C is one [rows x n] matrix, ldc == n) every 128-row tile t writes
 * stats_partial[(2t) * n + col] = mean of the tile's valid rows, stats_partial[(2t+1) * n + col] = their sum of
 * squared deviations -- the chunk format of hypel_col_stats_partial with chunk_rows = 128, ready for
 * hypel_bn_finalize(n_chunks = ceil(rows / 128), chunk_rows = 128).  No accumulate. */
int hypel_seg_gemm_stats_f32(const float* a, int64_t lda, int32_t trans_a, const float* b, int64_t ldb,
                             int32_t trans_b, float* c, int64_t ldc, int32_t n, const hypel_group_t* groups,
                             const hypel_seg_t* segs, const hypel_tile_t* tiles, int32_t n_tiles, const float* bias,
                             int32_t accumulate, float* stats_partial, hypel_stream_t stream);

/* hypel_seg_gemm_f32 with the shortcut gradient folded into the epilogue.  For `net = f(conv(net)) + scale_in_to_out(
 * net)` (nnmodel/HYPELCNNModel.py:160-163,176-183) the gradient of `net` is conv-data-gradient + transpose of the
 * channel map applied to dZ; instead of a separate gather pass plus a read-modify-write of the result, output
 * element (row, col) additionally receives sum_{o in [res_start[col], res_start[col+1])} res[row_abs * ldr + o],
 * row_abs = c_off / ldc + m0 + row (res has the row order of C: pixel-major).  res_start NULL = identity map. */
int hypel_seg_gemm_res_f32(const float* a, int64_t lda, int32_t trans_a, const float* b, int64_t ldb, int32_t trans_b,
                           float* c, int64_t ldc, int32_t n, const hypel_group_t* groups, const hypel_seg_t* segs,
                           const hypel_tile_t* tiles, int32_t n_tiles, const float* bias, int32_t accumulate,
                           const float* res, int64_t ldr, const int32_t* res_start, hypel_stream_t stream);

/* SEVERAL products C_p = A_p^T B_p in ONE launch -- the filter gradients of many layers (tf.gradients w.r.t. the
 * `weights` of every tf_slim.conv2d / fully_connected, common/common_nn_ops.py:232), which are mutually independent
 * and individually too small to fill 256 CUs: every launch pays ~25 us of ramp-up and drain, a step has twenty of
 * them.  `blocks` holds one record per 128 x tile_width output BLOCK: its group (rows, segment range, output offset,
 * first segment, as in hypel_tile_t) plus what used to be per-launch arguments -- column tile n0, the product's n,
 * lda, ldb, ldc -- and flags (bit 0 = accumulate into C).  Every offset (records and `segs`) is in elements relative
 * to `base`, one pointer for A, B and C (the operands live in different allocations; differences of device
 * addresses are exact in int64).  tile_width in {16, 32, 64} (| HYPEL_GEMM_MULTI_SPLIT6: {32, 64, 128}, the width of
 * the column tiles n0 the records were built for); trans_a = 1, trans_b = 0 only. */
typedef struct {
    int64_t c_off; int64_t a_off0; int64_t b_off0;      /* output offset of the group; segs[seg_begin] copy */
    int32_t m0; int32_t rows; int32_t n0; int32_t n;      /* output rows [m0, m0+128) x columns [n0, n0+tile_width) */
    int32_t seg_begin; int32_t seg_count; int32_t k0; int32_t flags;
    int32_t lda; int32_t ldb; int32_t ldc; int32_t reserved;
} hypel_mtile_t;
int hypel_seg_gemm_multi_f32(const float* base, int32_t trans_a, int32_t trans_b, int32_t tile_width,
                             const hypel_seg_t* segs, const hypel_mtile_t* blocks, int32_t n_blocks,
                             hypel_stream_t stream);

/* Several hypel_reduce_splits_f32 in one launch (the second stage of the merged filter-gradient launch):
 * entry e: out_e[i] = (flags_e & 1 ? out_e[i] : 0) + sum_{s < n_splits_e} partial_e[s*stride_e + i], i < count_e;
 * partial_off / out_off in elements relative to `base`. */
typedef struct {
    int64_t partial_off; int64_t out_off; int64_t stride; int64_t count; int32_t n_splits; int32_t flags;
} hypel_reduce_entry_t;
int hypel_reduce_splits_multi_f32(const float* base, const hypel_reduce_entry_t* entries, int32_t n_entries,
                                  hypel_stream_t stream);
/* The same reduction when the caller knows max_count = the largest entry's count: the grid is sized for it (the K-slice
 * partials of a GEMM launch, HYPEL_TILE_PLAIN: many entries of one 128-row tile each).  Same sums, same order. */
int hypel_reduce_splits_multi_sized_f32(const float* base, const hypel_reduce_entry_t* entries, int32_t n_entries,
                                        int64_t max_count, hypel_stream_t stream);

/* The same table for reductions with MANY slabs and few outputs (the per-block gradient slabs that the fused
 * generator / dense-stack backward kernels of one GAN train op leave: all of them in one launch): one wavefront per
 * output element, lanes over the slabs; total_count = sum of the entries' counts (host knowledge: sizes the grid).
 * Two entries of one launch must not write the same output. */
int hypel_reduce_splits_wave_multi_f32(const float* base, const hypel_reduce_entry_t* entries, int32_t n_entries,
                                       int64_t total_count, hypel_stream_t stream);

/* out[o(i)] = (accumulate ? out[o(i)] : 0) + (bias ? bias[i mod n] : 0) + sum_s partial[s*stride + o(i)], s ascending
 * (deterministic second stage of every split launch: filter gradients, FC-shaped products whose output has too
 * few tiles to fill 256 CUs, and the tap-split heavy branches of a multi-kernel level).
 * ldc <= 0: o(i) = i (dense).  ldc > 0: o(i) = (i / n) * ldc + i mod n, a [count/n x n] window of a wider matrix. */
int hypel_reduce_splits_f32(const float* partial, int64_t stride, int32_t n_splits, float* out, int64_t count,
                            int32_t accumulate, const float* bias, int32_t n, int64_t ldc, hypel_stream_t stream);

/* Two hypel_reduce_splits_f32 (dense, no bias) over the same n_splits slabs in one launch -- the filter and the bias
 * gradients a fused stack (hypel_gan_generator_bwd, hypel_dense_stack_bwd) leaves per block; bit-identical to the two
 * separate calls. */
int hypel_reduce_splits_pair_f32(const float* partial0, int64_t stride0, int64_t count0, float* out0,
                                 const float* partial1, int64_t stride1, int64_t count1, float* out1, int32_t n_splits,
                                 int32_t accumulate, hypel_stream_t stream);

/* 2-D block copies in one launch: entry e copies (or adds) a [rows x cols] block, dst[dst_off + r * dst_ld + c]
 * (+)= src[src_off + r * src_ld + c]; offsets in elements relative to `base` (one pointer for every operand, as in
 * hypel_seg_gemm_multi_f32), flags bit 0 = accumulate.  Builds the packed weight image of a merged multi-kernel level
 * from its tf_slim.conv2d HWIO variables (one entry per (branch, tap): the [Cin x cout] slice goes to offset d, columns
 * [branch * cout, (branch + 1) * cout) of W_pack) before the forward pass, and scatters the packed filter gradient back
 * into the variables' gradient slots after the backward pass -- TF names and layouts stay at the boundary.  Also gathers
 * the inputs of same-weight GAN applications into one row-concatenated batch (cut_wrapper.py:301-339) and scatters its
 * gradient back.  max_block_elems = rows * cols of the largest entry (host knowledge: sizes the grid). */
typedef struct {
    int64_t src_off; int64_t dst_off; int32_t rows; int32_t cols; int32_t src_ld; int32_t dst_ld; int32_t flags;
    int32_t reserved;
} hypel_copy_block_t;
int hypel_copy_blocks_f32(const float* base, const hypel_copy_block_t* entries, int32_t n_entries,
                          int64_t max_block_elems, hypel_stream_t stream);
/* Two flat copies in one launch, dst_i[0 .. n_i) = src_i[0 .. n_i) (n1 may be 0): the two batches a GAN train op is fed
 * with (x and y, resp. the two tensor-pool results of the critics' phase; gan/wrappers/gan_common.py run_step) -- each
 * copy launch of a 0.28 ms CycleGAN step is 1.7 % of it. */
int hypel_copy_pair_f32(float* dst0, const float* src0, int64_t n0, float* dst1, const float* src1, int64_t n1,
                        hypel_stream_t stream);

/* ---- batch norm statistics (tf_slim.batch_norm fused, HYPELCNNModel.py:37,43-44) ------------------
 * partial[chunk][0][c] = mean of the chunk's rows, partial[chunk][1][c] = sum of squared deviations.
 * chunk = `chunk_rows` consecutive rows (last may be short). */
int hypel_col_stats_partial(const float* x, int64_t ld, int64_t rows, int32_t c, int32_t chunk_rows, float* partial,
                            hypel_stream_t stream);
/* Chan-merge the chunk partials in chunk order (fp64) -> mean[c], rstd[c] = 1/sqrt(var_biased+eps);
 * optional moving-average update m <- m*decay + batch*(1-decay) with the Bessel-corrected variance. */
int hypel_bn_finalize(const float* partial, int32_t n_chunks, int32_t chunk_rows, int64_t rows, int32_t c, float eps,
                      float* mean, float* rstd, float* moving_mean, float* moving_var, float decay,
                      hypel_stream_t stream);
/* Synchronised batch norm across data-parallel ranks (optional; the reference is single-device, so this is what makes
 * N ranks x nb equal the reference's one device at batch N x nb -- tf_slim.batch_norm, HYPELCNNModel.py:37,43):
 * a rank merges its chunk partials into one record out[0..c) = mean, out[c..2c) = sum of squared deviations,
 * out[2c] = rows; the host all-gathers the records (RCCL); hypel_bn_finalize_ranks merges `world` records
 * ([world][2c+1], rank order, fp64) into mean / rstd / moving averages -- identical on every rank. */
int hypel_bn_merge_partials(const float* partial, int32_t n_chunks, int32_t chunk_rows, int64_t rows, int32_t c,
                            float* out, hypel_stream_t stream);
int hypel_bn_finalize_ranks(const float* gathered, int32_t world, int32_t c, float eps, float* mean, float* rstd,
                            float* moving_mean, float* moving_var, float decay, hypel_stream_t stream);
int hypel_bn_act_small_fwd(const float* y, int64_t ldy, int64_t rows, int32_t c, float eps, const float* beta,
                           int32_t act, float alpha, const float* mask, int64_t ldm, float* mean, float* rstd,
                           float* moving_mean, float* moving_var, float decay, float* z, int64_t ldz,
                           hypel_stream_t stream);
int hypel_bn_act_small_bwd(const float* dz, int64_t lddz, const float* y, int64_t ldy, int64_t rows, int32_t c,
                           const float* mean, const float* rstd, const float* beta, int32_t act, float alpha,
                           const float* mask, int64_t ldm, float* dy, int64_t lddy, float* dparam,
                           int32_t accumulate, hypel_stream_t stream);
/* inference: rstd[c] = 1/sqrt(moving_var[c] + eps) */
int hypel_rstd_from_var(const float* var, int32_t c, float eps, float* rstd, hypel_stream_t stream);

/* ---- fused post-op: z = act((y - mean) * rstd + beta) * mask + res1[:, idx1] + res2[:, idx2] ---------
 * mean/rstd/beta NULL -> no normalisation (bias was added by the GEMM).  mask NULL -> no dropout
 * (tf_slim.dropout, HYPELCNNModel.py:123).  idx NULL -> identity channel map; otherwise the
 * scale_in_to_out gather/repeat index vector (common_nn_ops.py:546-564). */
int hypel_bn_act_fwd(const float* y, int64_t ldy, int64_t rows, int32_t c, const float* mean, const float* rstd,
                     const float* beta, int32_t act, float alpha, const float* mask, int64_t ldm, const float* res1,
                     int64_t ld1, const int32_t* idx1, const float* res2, int64_t ld2, const int32_t* idx2, float* z,
                     int64_t ldz, hypel_stream_t stream);
/* backward pass 1: partial[chunk][0][c] = sum dyh, partial[chunk][1][c] = sum dyh*xhat over the chunk rows,
 * dyh = dz*mask*act'(yh).  (xhat := y when there is no normalisation.) */
int hypel_bn_act_bwd_reduce(const float* dz, int64_t lddz, const float* y, int64_t ldy, int64_t rows, int32_t c,
                            const float* mean, const float* rstd, const float* beta, int32_t act, float alpha,
                            const float* mask, int64_t ldm, int32_t chunk_rows, float* partial, hypel_stream_t stream);
/* sums[0][c] = sum over chunks (fp64, chunk order) of partial[.][0][c]; sums[1][c] likewise;
 * dparam (beta or bias gradient) = sums[0] (+= when accumulate). */
int hypel_bwd_reduce_finalize(const float* partial, int32_t n_chunks, int32_t c, float* sums, float* dparam,
                              int32_t accumulate, hypel_stream_t stream);
/* hypel_bn_act_bwd_reduce for a layer WITHOUT batch norm (tf_slim.fully_connected / conv2d with biases:
 * shadow_data_models.py:95-146, DUALCNNModel.py:48-54,99-100) that ALSO writes dY = dZ * act'(y) (* mask): there dY
 * needs no column sum, so the pass that reduces the bias gradient delivers it and hypel_bn_act_bwd_apply (one more read
 * of dZ and Y, one more launch) is not needed.  partial as hypel_bn_act_bwd_reduce (finish with
 * hypel_bwd_reduce_finalize); dy may alias dz. */
int hypel_act_bias_bwd_reduce(const float* dz, int64_t lddz, const float* y, int64_t ldy, int64_t rows, int32_t c,
                              int32_t act, float alpha, const float* mask, int64_t ldm, int32_t chunk_rows, float* partial,
                              float* dy, int64_t lddy, hypel_stream_t stream);
/* backward pass 2: dy = rstd*(dyh - sums0/M - xhat*sums1/M)   (or dy = dyh without normalisation).
 * dy may alias dz. */
int hypel_bn_act_bwd_apply(const float* dz, int64_t lddz, const float* y, int64_t ldy, int64_t rows, int32_t c,
                           const float* mean, const float* rstd, const float* beta, int32_t act, float alpha,
                           const float* mask, int64_t ldm, const float* sums, float* dy, int64_t lddy,
                           hypel_stream_t stream);
/* the same with M = stat_rows >= rows: the sums were all-reduced over the data-parallel ranks and run over the global
 * batch (synchronised batch norm, see hypel_bn_merge_partials). */
int hypel_bn_act_bwd_apply_global(const float* dz, int64_t lddz, const float* y, int64_t ldy, int64_t rows, int32_t c,
                                  const float* mean, const float* rstd, const float* beta, int32_t act, float alpha,
                                  const float* mask, int64_t ldm, const float* sums, int64_t stat_rows, float* dy,
                                  int64_t lddy, hypel_stream_t stream);
/* gradient of the channel map: dr[row][ci] (+)= sum_{c in [start[ci], start[ci+1])} dz[row][c];
 * start NULL -> identity (cin == c). */
int hypel_chanmap_bwd(const float* dz, int64_t lddz, int64_t rows, int32_t c, float* dr, int64_t lddr, int32_t cin,
                      const int32_t* start, int32_t accumulate, hypel_stream_t stream);

/* ---- losses ------------------------------------------------------------------------------------------ */
/* tf.nn.softmax_cross_entropy_with_logits (HYPELCNNModel.py:102, DUALCNNModel.py:88, cut_wrapper.py:382,413):
 * loss[i] = -sum_j labels[i][j]*log_softmax(logits[i])[j];
 * dlogits[i][j] = gscale*(softmax[i][j]*sum_j labels[i][j] - labels[i][j])  (dlogits NULL -> skipped). */
int hypel_softmax_xent(const float* logits, int64_t ld, int64_t n, int32_t c, const float* labels, int64_t ldl,
                       float* loss, float* dlogits, int64_t lddl, float gscale, hypel_stream_t stream);
/* reconstruction MSE (HYPELCNNModel.py:106-109): out[0] = mean((a-b)^2) over rows x c;
 * da = gscale*2*(a-b)/(rows*c) (da NULL -> skipped).  ws: >= 1024 floats. */
int hypel_mse(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int32_t c, float* out, float* da,
              int64_t ldda, float gscale, float* ws, hypel_stream_t stream);
/* The classifier's loss tail in two launches instead of six (HYPELCNNModel.py:101-112: softmax cross entropy + weighted
 * reconstruction MSE; NanTensorHook, monitored_session_runner.py:151):
 * hypel_mse_partial_f32 = first stage of hypel_mse -- da as there, ws[HYPEL_MSE_PARTIALS] = per-block sums of squares;
 * hypel_loss_finalize_f32: out_ce = mean(loss_rows[n_rows]) (the per-row values hypel_softmax_xent wrote),
 * out_mse = sum(mse_ws) * mse_scale (both NULL = no reconstruction term), flag = 1.0f if either is not finite else 0
 * (NULL = no guard; same flag as hypel_loss_guard_f32), *step += 1 (NULL = leave; same as hypel_step_inc). */
#define HYPEL_MSE_PARTIALS 1024
int hypel_mse_partial_f32(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int32_t c, float* da,
                          int64_t ldda, float gscale, float* ws, hypel_stream_t stream);
int hypel_loss_finalize_f32(const float* loss_rows, int32_t n_rows, const float* mse_ws, double mse_scale, float* out_ce,
                            float* out_mse, float* flag, uint64_t* step, hypel_stream_t stream);

/* out[0] = sum(x[0..count)) * scale, deterministic two-stage.  ws >= 1024 floats. */
int hypel_sum_f32(const float* x, int64_t count, float scale, float* out, float* ws, hypel_stream_t stream);

/* ---- optimisers (common_nn_ops.py:223-230; gan_common.py:264-265) ---------------------------------------- */
/* TF1 Adam: m=b1*m+(1-b1)g; v=b2*v+(1-b2)g^2; p -= lr_t*m/(sqrt(v)+eps), lr_t precomputed on the host. */
int hypel_adam_tf1(float* p, const float* g, float* m, float* v, int64_t count, float lr_t, float beta1, float beta2,
                   float eps, hypel_stream_t stream);
/* TF1 Momentum: a = mu*a + g; p -= lr*a. */
int hypel_momentum_tf1(float* p, const float* g, float* a, int64_t count, float lr, float mu, hypel_stream_t stream);
/* Non-finite loss guard -- NanTensorHook (classify/monitored_session_runner.py:151) + check_numerics inside
 * create_train_op (common/common_nn_ops.py:232), moved onto the device so that the step loop never waits for
 * the loss: flag[0] = 1.0f if loss_a[0] (or loss_b[0], nullable) is NaN/Inf, else 0.0f.  The session keeps
 * the flag in the element BEHIND the flat gradient buffer, so the data-parallel all-reduce (sum) of the gradients
 * gives every rank the same verdict.  The *_guarded optimisers return without touching p / slots when
 * skip[0] != 0 (skip NULL = unguarded). */
int hypel_loss_guard_f32(const float* loss_a, const float* loss_b, float* flag, hypel_stream_t stream);
int hypel_adam_tf1_guarded(float* p, const float* g, float* m, float* v, int64_t count, float lr_t, float beta1,
                           float beta2, float eps, const float* skip, hypel_stream_t stream);
int hypel_momentum_tf1_guarded(float* p, const float* g, float* a, int64_t count, float lr, float mu, const float* skip,
                               hypel_stream_t stream);

/* ---- dropout mask (tf_slim.dropout): mask in {0, 1/keep}, Philox4x32-10 counter RNG ----------------------
 * counter = (element group, *step_dev), key = seed: the step lives on the device so that a captured
 * HIP graph draws fresh masks on every replay; hypel_step_inc bumps it once per training step. */
int hypel_dropout_mask(float* mask, int64_t count, float keep_prob, uint64_t seed, const uint64_t* step_dev,
                       hypel_stream_t stream);
int hypel_step_inc(uint64_t* step_dev, hypel_stream_t stream);

/* ---- evaluation (common_nn_ops.py:243-277): pred[i] = argmax logits[i] (first max, as tf.argmax);
 * confusion[label][pred] += 1 (int32 atomics; the table is not cleared, a second call accumulates). labels: int32 class
 * ids; a row whose label lies outside [0, c) -- -1, c, the raster's "unknown" 255 -- is not counted (its pred is still
 * written).  pred may be NULL; confusion or labels NULL -> nothing is counted.
 * The argmax of hypel_argmax_confusion and hypel_argmax_scatter is one left-to-right pass that starts at column 0 and
 * moves on `logits[i][j] > best` (strict): of equal maxima (+0 and -0 are equal) the first wins; a NaN never displaces a
 * value, and a NaN in column 0 is never displaced -- [1, NaN, 3] gives 2, [NaN, 5] gives 0, an all-NaN row gives 0.  (Not
 * numpy.argmax, where the first NaN wins.)  The label of a row with a NaN means nothing; the rule is fixed so that
 * device and specification cannot differ on it. */
int hypel_argmax_confusion(const float* logits, int64_t ld, int64_t n, int32_t c, const int32_t* labels,
                           int32_t* pred, int32_t* confusion, hypel_stream_t stream);

/* ---- data side: scene -> patches -> augmented batch; predictions -> label raster ---------------------------
 * hypel_gather_patches_f32 replaces the per-target Python loop over BasicDataSet.get_data_point
 * (common_nn_ops.py:169-185; importer/InMemoryImporter.py:27-38; importer/GeneratorImporter.py): casi
 * [hp, wp, cc] and lidar [hp, wp, cl] (NULL when cl == 0) are the symmetric-padded, normalised scene in HBM;
 * points int32 [n, 2] = (x, y) of the target = window origin in the padded scene; out [n, p, p, cc + cl].
 *
 * hypel_augment_patches_f32 replaces the tf.data map stage (common_nn_ops.py:376-440) and the batch gather in
 * front of it: for sample s, source = x[idx[s]] (idx NULL = identity), rotated counter-clockwise by rot_k[s]
 * quarter turns (the reference draws k in {0,1,2}, :402), shadowed when shadow_pick[s] (by division with
 * shadow_ratio[c] -- create_simple_shadow_struct, gan_utilities.py:17-27 -- or by taking the sample from
 * shadow_alt [n,p,p,c], the pre-computed generator output in batch order), flipped left/right and up/down when
 * flip_lr[s] / flip_ud[s], shifted by delta[s, c] (spectral augmentation).  Every selector may be NULL.  The random
 * decisions are drawn by the host iterator (seeded generator) and handed over as small device arrays.  shadow_ratio
 * and shadow_alt are two definitions of the same step: a call that gives both is refused (as is shadow_pick with
 * neither), before anything is written.
 *
 * hypel_argmax_scatter replaces perform_prediction's per-sample Python loop (common_nn_ops.py:313-327):
 * raster[y * raster_w + x] = argmax(logits[i]) for points[i] = (x, y). */
int hypel_gather_patches_f32(const float* casi, const float* lidar, int64_t hp, int64_t wp, int32_t cc, int32_t cl,
                             const int32_t* points, int64_t n, int32_t p, float* out, hypel_stream_t stream);
/* GRSS2018DataSet.get_data_point (loader/GRSS2018DataLoader.py:12-44): casi [*, casi_wp, cc] has half the
 * resolution of lidar [*, lidar_wp, cl]; both are padded by `neighborhood`; points are LiDAR-grid coordinates. */
int hypel_gather_patches_2x_f32(const float* casi, const float* lidar, int64_t casi_wp, int64_t lidar_wp, int32_t cc,
                                int32_t cl, int32_t neighborhood, const int32_t* points, int64_t n, int32_t p,
                                float* out, hypel_stream_t stream);
int hypel_augment_patches_f32(const float* x, const int64_t* idx, int64_t n, int32_t p, int32_t c,
                              const int32_t* rot_k, const uint8_t* shadow_pick, const float* shadow_ratio,
                              const float* shadow_alt, const uint8_t* flip_lr, const uint8_t* flip_ud,
                              const float* delta, float* out, hypel_stream_t stream);
int hypel_argmax_scatter(const float* logits, int64_t ld, int64_t n, int32_t c, const int32_t* points,
                         uint8_t* raster, int64_t raster_w, hypel_stream_t stream);
/* The GAN trainer's tf.data stage (gan/gan_train_for_shadow.py:147-182: from_tensor_slices -> shuffle_and_repeat ->
 * map(perform_shadow_augmentation_random) -> batch): pair i of the batch = (normal[idx[i]], shadow[idx[i]]), both
 * [pool][bands] resident in HBM; with ratio != NULL the regulariser swap of :171-182 -- u1[i] < rate replaces the normal
 * spectrum by shadow * ratio, u2[i] < rate then replaces the shadow spectrum by (the possibly replaced) normal / ratio;
 * u1 / u2 are the two uniform draws per pair (host RNG, the reference's tf.random.uniform([1], 0.01, 0.99)). */
int hypel_gather_pairs_f32(const float* normal, const float* shadow, const int64_t* idx, int64_t n, int32_t bands,
                           const float* ratio, const float* u1, const float* u2, float rate, float* out_x, float* out_y,
                           hypel_stream_t stream);
/* The GAN scene conversion's write-back (gan/gan_infer_image_for_shadow.py:84-85, ((g * casi_max) + casi_min)
 * .astype(dtype) per pixel): out[rows[i] * ld_out + b] = cast(src[i * ld_src + b] * scale[b] + offset[b]) for i < n,
 * b < bands; rows NULL = identity.  Multiply and add are rounded separately (no fma), as NumPy's float32 operators.
 * cast: float32 as is; the integer dtypes as NumPy on x86-64 -- truncation to int32 (NaN, +-inf and out-of-range
 * values give INT_MIN), then the low bits.  out_dtype: HYPEL_DTYPE_*. */
enum { HYPEL_DTYPE_F32 = 0, HYPEL_DTYPE_U16 = 1, HYPEL_DTYPE_I16 = 2, HYPEL_DTYPE_U8 = 3 };
int hypel_denorm_scatter(const float* src, int64_t ld_src, const int64_t* rows, int64_t n, int32_t bands,
                         const float* scale, const float* offset, int32_t out_dtype, void* out, int64_t ld_out,
                         hypel_stream_t stream);
/* The sRGB rendering of a raster (common/hsi_rgb_converter.py get_rgb_from_hsi with the CIE 1931 2 degree observer and
 * illuminant E, as gan/gan_infer_image_for_shadow.py:97-104 applies it to the converted scene): raster [n_pixels][ld_in]
 * of in_dtype (HYPEL_DTYPE_*), of which the bands band0 .. band0 + span - 1 <= bands - 1 are read.  table [span][4]
 * float64, 32-byte aligned: {offset, wx, wy, wz} per band of the span, so that
 *   XYZ = sum_b (raster[p][band0 + b] - offset[b]) * (wx, wy, wz)[b]
 * is the reference's XYZ / 100 -- the caller folds the 31 selected bands (duplicates summed, unselected bands zero),
 * the colour matching functions, 1 / sum(ybar) and 1 / casi_max into the weights.  Then skimage's xyz2rgb: the inverse
 * of [[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]],
 * 1.055 * lin^(1/2.4) - 0.055 above 0.0031308 and 12.92 * lin below, clipped to [0, 1].  The sums and the matrix are
 * float64, the curve is float32 (within 1e-6).  out [n_pixels][3]: float32 rgb (HYPEL_RGB_F32, levels unused), or uint8
 * trunc(255 * rgb) (HYPEL_RGB_U8): levels [256] float64 with levels[0] = -inf and levels[k] the smallest linear value
 * whose float64 curve times 255 reaches k, so that the byte is the largest k with levels[k] <= lin, exactly.  Inputs
 * are finite: a pixel with a non-finite sample anywhere in its span renders as 0. */
enum { HYPEL_RGB_U8 = 0, HYPEL_RGB_F32 = 1 };
int hypel_hsi_to_srgb(const void* raster, int32_t in_dtype, int64_t ld_in, int64_t n_pixels, int32_t bands,
                      int32_t band0, int32_t span, const double* table, const double* levels, int32_t out_mode,
                      void* out, hypel_stream_t stream);

/* ---- LRN (tf.nn.local_response_normalization, CONCNNModel.py:37,41) -------------------------------------- */
int hypel_lrn_fwd(const float* x, int64_t ldx, int64_t rows, int32_t c, int32_t radius, float bias, float alpha,
                  float beta, float* y, int64_t ldy, hypel_stream_t stream);
int hypel_lrn_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t rows, int32_t c, int32_t radius,
                  float bias, float alpha, float beta, float* dx, int64_t lddx, int32_t accumulate,
                  hypel_stream_t stream);

/* ---- shadow GAN stacks (gan/shadow_data_models.py, gan/wrappers/) -------------------------------------------
 * Fused generator (shadowdata_generator_model :43-90): x[N][B] -> out[N][B]; seven 1-channel SAME 1-D convolutions
 * over the band axis with kernel sizes B, B/2, B/4, B/8, B/4, B/2, B, leaky-ReLU(0.1), skip sums
 * n_i = c_i + n_{i-1} + n_{i-2}, tanh on the last layer; only_encoder != 0 stops after layer 4 and returns n4.
 * w = the layers' kernels concatenated (TF variables netK/weights [k,1,1]), b = 7 biases.  From 16 to 368 bands (the
 * largest count whose backward images fit the 160 KB of LDS) the stack runs on the matrix cores
 * (csrc/gan_mfma.hip: a 1-channel SAME convolution over B bands of N samples is
 * X[N x B] . T[B x B] with T banded Toeplitz; 16 samples per block, activations in LDS, the taps as the MFMA B operand
 * straight from a zero-margined table, filter gradient = diagonal sums of X^T dZ tiles accumulated per tile offset);
 * otherwise one wavefront (or two) per sample on the vector ALUs (csrc/gan.hip).  The backward recomputes the forward;
 * weight / bias gradients are written as per-block partial sums pw[blocks][sum k], pb[blocks][8] with
 * blocks = hypel_gan_generator_blocks(n) (reduce with hypel_reduce_splits_f32; every slab is written).  dx may be NULL. */
int hypel_gan_generator_blocks(int64_t n);
int hypel_gan_generator_fwd(const float* x, int64_t ldx, int64_t n, int32_t bands, const float* w, const float* b,
                            int32_t only_encoder, float* out, int64_t ldo, hypel_stream_t stream);
int hypel_gan_generator_bwd(const float* x, int64_t ldx, const float* dout, int64_t lddo, int64_t n, int32_t bands,
                            const float* w, const float* b, int32_t only_encoder, float* dx, int64_t lddx,
                            int32_t accumulate_dx, float* pw, float* pb, hypel_stream_t stream);

/* The same pair with the forward pass's activations KEPT for the backward pass instead of recomputed there (29 % of the
 * matrix-core backward kernel at B = 360): hypel_gan_generator_fwd_keep leaves the layer outputs, leaky-ReLU branch bits and
 * the tanh output of every 16-sample tile in `keep` (hypel_gan_generator_keep_floats(n, bands, only_encoder) floats; an
 * opaque, lane-native layout), hypel_gan_generator_bwd_kept of the SAME (x, w, b, n, bands, only_encoder) starts from it:
 * bit-identical to the recomputing pair.  keep_floats == 0: this band count runs on the VALU kernels, which always
 * recompute -- pass keep = NULL (then the calls are hypel_gan_generator_fwd / _bwd). */
int64_t hypel_gan_generator_keep_floats(int64_t n, int32_t bands, int32_t only_encoder);
/* Encoder tap (round 4).  CUT applies the encoder-only generator to tensors the FULL generator of the same train op also
 * consumes (gan/wrappers/cut_wrapper.py:301-339: gen(x), gen(x, only_encoder) -- and the same for y): the encoder output is
 * the full generator's n_4.  hypel_gan_generator_fwd_tap = hypel_gan_generator_fwd[_keep](only_encoder = 0) that also writes
 * enc_out[n x bands] = what hypel_gan_generator_fwd(only_encoder = 1) would write, bit for bit (keep may be NULL);
 * hypel_gan_generator_bwd_tap = hypel_gan_generator_bwd[_kept](only_encoder = 0) that adds d_enc -- the gradient of enc_out
 * -- to the gradient of n_4: one backward pass yields the input and filter gradients of both applications.
 * Matrix-core kernels only: hypel_gan_generator_tap_supported(bands) != 0. */
int hypel_gan_generator_tap_supported(int32_t bands);
int hypel_gan_generator_fwd_tap(const float* x, int64_t ldx, int64_t n, int32_t bands, const float* w, const float* b,
                                float* out, int64_t ldo, float* enc_out, int64_t ld_enc, float* keep,
                                hypel_stream_t stream);
int hypel_gan_generator_bwd_tap(const float* x, int64_t ldx, const float* dout, int64_t lddo, const float* d_enc,
                                int64_t ld_denc, int64_t n, int32_t bands, const float* w, const float* b, float* dx,
                                int64_t lddx, int32_t accumulate_dx, float* pw, float* pb, const float* keep,
                                hypel_stream_t stream);
int hypel_gan_generator_fwd_keep(const float* x, int64_t ldx, int64_t n, int32_t bands, const float* w, const float* b,
                                 int32_t only_encoder, float* out, int64_t ldo, float* keep, hypel_stream_t stream);
int hypel_gan_generator_bwd_kept(const float* x, int64_t ldx, const float* dout, int64_t lddo, int64_t n, int32_t bands,
                                 const float* w, const float* b, int32_t only_encoder, float* dx, int64_t lddx,
                                 int32_t accumulate_dx, float* pw, float* pb, const float* keep, hypel_stream_t stream);

/* ---- a short stack of narrow fully-connected layers in one launch per direction ------------------------------------
 * shadowdata_discriminator_model (gan/shadow_data_models.py:95-121): flatten -> tf_slim.fully_connected B -> B -> B -> B/2
 * with biases, leaky-ReLU(0.1) on the first two.  When every width is <= 128 (the Gulfport stacks, B = 64) the whole stack
 * of one application runs out of LDS, 16 samples per block, on v_mfma_f32_16x16x4_f32 -- instead of one GEMM + one
 * activation launch per layer forward and ~12 launches backward, each a few microseconds of launch latency.
 *   n_layers <= 4, widths w0 -> w1 -> ... (unused trailing widths 0); bit l of act_mask: leaky-ReLU(alpha) after layer l.
 *   w: the layers' [cin][cout] matrices one after the other (tf_slim `weights`), b: their biases one after the other.
 *   bwd: recomputes the forward; dx may be NULL; pw[blocks][sum cin*cout] / pb[blocks][sum cout] are per-block partial
 *   filter / bias gradients, blocks = hypel_dense_stack_blocks(n) -- every slab is written; sum them in slab order with
 *   hypel_reduce_splits_f32 (deterministic).  hypel_dense_stack_supported: 1 when the shape runs here. */
int hypel_dense_stack_supported(int32_t n_layers, int32_t w0, int32_t w1, int32_t w2, int32_t w3, int32_t w4);
int hypel_dense_stack_blocks(int64_t n);
int hypel_dense_stack_fwd(const float* x, int64_t ldx, int64_t n, int32_t n_layers, int32_t w0, int32_t w1, int32_t w2,
                          int32_t w3, int32_t w4, int32_t act_mask, float alpha, const float* w, const float* b, float* out,
                          int64_t ldo, hypel_stream_t stream);
int hypel_dense_stack_bwd(const float* x, int64_t ldx, const float* dout, int64_t lddo, int64_t n, int32_t n_layers,
                          int32_t w0, int32_t w1, int32_t w2, int32_t w3, int32_t w4, int32_t act_mask, float alpha,
                          const float* w, const float* b, float* dx, int64_t lddx, int32_t accumulate_dx, float* pw,
                          float* pb, hypel_stream_t stream);

/* ---- several applications of same-shaped networks with DIFFERENT variables in one launch -----------------------------
 * CycleGAN applies two generators (x2y, y2x) and two critics (D_x, D_y) of one shape side by side
 * (gan/wrappers/cycle_gan_wrapper.py:82-124; the DCL-GAN pair of CUT models likewise): at the Gulfport sizes every such
 * application is a latency chain that leaves most of the chip idle, so application g of `n_apps` runs on its own share of
 * the blocks of ONE launch.  Rows: application g reads rows [g*n, (g+1)*n) of x / dout / keep and writes the same rows of
 * out / dx (n rows per application).  Variables: application g's are at w + g*w_stride, b + g*b_stride (elements; any
 * sign -- the variables of two models lie a fixed distance apart in the flat parameter buffer).  Gradient slabs (bwd):
 * blocks_apps(n, n_apps) / n_apps slabs per application, application g's first slab at pw + g*pw_stride, pb + g*pb_stride
 * (pw_stride == 0: all slabs consecutive in application order).  Each application's results are bit-identical to the
 * single-application entry point's on its rows, and its slabs sum to the same gradients.
 * Generator: matrix-core shapes only (hypel_gan_generator_tap_supported(bands)); keep (nullable) holds
 * n_apps * hypel_gan_generator_keep_floats(n) floats, application after application. */
int hypel_gan_generator_blocks_apps(int64_t n, int32_t n_apps);
int hypel_gan_generator_fwd_apps(const float* x, int64_t ldx, int64_t n, int32_t n_apps, int64_t w_stride, int64_t b_stride,
                                 int32_t bands, const float* w, const float* b, int32_t only_encoder, float* out,
                                 int64_t ldo, float* keep, hypel_stream_t stream);
int hypel_gan_generator_bwd_apps(const float* x, int64_t ldx, const float* dout, int64_t lddo, int64_t n, int32_t n_apps,
                                 int64_t w_stride, int64_t b_stride, int64_t pw_stride, int64_t pb_stride, int32_t bands,
                                 const float* w, const float* b, int32_t only_encoder, float* dx, int64_t lddx,
                                 int32_t accumulate_dx, float* pw, float* pb, const float* keep, hypel_stream_t stream);
int hypel_dense_stack_blocks_apps(int64_t n, int32_t n_apps);
int hypel_dense_stack_fwd_apps(const float* x, int64_t ldx, int64_t n, int32_t n_apps, int64_t w_stride, int64_t b_stride,
                               int32_t n_layers, int32_t w0, int32_t w1, int32_t w2, int32_t w3, int32_t w4,
                               int32_t act_mask, float alpha, const float* w, const float* b, float* out, int64_t ldo,
                               hypel_stream_t stream);
int hypel_dense_stack_bwd_apps(const float* x, int64_t ldx, const float* dout, int64_t lddo, int64_t n, int32_t n_apps,
                               int64_t w_stride, int64_t b_stride, int64_t pw_stride, int64_t pb_stride, int32_t n_layers,
                               int32_t w0, int32_t w1, int32_t w2, int32_t w3, int32_t w4, int32_t act_mask, float alpha,
                               const float* w, const float* b, float* dx, int64_t lddx, int32_t accumulate_dx, float* pw,
                               float* pb, hypel_stream_t stream);

/* tensorflow_gan losses: mode 0: weight*mean((a-target)^2) (least squares, pass weight/2),
 * mode 1: weight*mean(|a-b|) (cycle consistency / absolute_difference), mode 2: weight*mean(a) (Wasserstein).
 * loss[0] (+)= value; da / db (nullable) (+)= gradient.  ws >= 1024 floats. */
int hypel_gan_loss(int32_t mode, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int32_t c,
                   float target, float weight, float* loss, int32_t accumulate_loss, float* da, int64_t ldda,
                   int32_t acc_da, float* db, int64_t lddb, int32_t acc_db, float* ws, hypel_stream_t stream);
/* tf_slim.l2_regularizer: loss[0] (+)= scale/2 * sum w^2 ; dw (nullable) += scale * w.  ws >= 1024 floats. */
int hypel_l2_reg(const float* w, int64_t count, float scale, float* loss, int32_t accumulate_loss, float* dw,
                 float* ws, hypel_stream_t stream);

/* The same terms with a DEFERRED sum: every loss term of a train op (tfgan tuple losses, cycle / identity L1, the scope's
 * l2 regularisers) leaves its weighted block partials in its own slot of 1024 floats (hypel_loss_terms_slots); ONE
 * hypel_loss_finalize_slots at the end of the op adds slots [0, n_slots) in index order into the op's loss -- one
 * finaliser launch per op instead of one per term. */
int hypel_loss_finalize_slots(const float* slots, int32_t n_slots, float* loss, int32_t accumulate_loss,
                              hypel_stream_t stream);

/* Several of those terms in ONE launch.  Offsets are in elements relative to `base` (HYPEL_LOSS_NONE = operand absent);
 * mode 0-2 as hypel_gan_loss (gcoef = weight / (rows * c), pscale = the same), mode 3 = hypel_l2_reg (a = w, rows =
 * count, da = dw, gcoef = scale, pscale = scale / 2).  Two terms of one launch must not write the same gradient buffer. */
#define HYPEL_LOSS_NONE INT64_MIN
typedef struct {
    int64_t a_off, b_off, da_off, db_off;
    int64_t lda, ldb, ldda, lddb, rows;
    int32_t mode, c, acc_da, acc_db;
    float target, gcoef, pscale;
    int32_t slot;
} hypel_loss_term_t;
int hypel_loss_terms_slots(const float* base, const hypel_loss_term_t* terms, int32_t n_terms, float* slots,
                           hypel_stream_t stream);
/* tf.math.l2_normalize(axis=None) over the whole [rows x c] tensor (shadow_data_models.py:147).
 * stat[0] = sum x^2, stat[1] = rsqrt(max(sum, 1e-12)). */
/* `parts` adjacent [rows x c] column blocks of one matrix, each normalised by its own whole-block norm, in one
 * launch (the stacked slice embeddings of the feature discriminator); stat holds 2 floats per part. */
int hypel_l2norm_parts_fwd(const float* x, int64_t ldx, int64_t rows, int32_t c, int32_t parts, float* y, int64_t ldy,
                           float* stat, hypel_stream_t stream);
int hypel_l2norm_parts_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t rows, int32_t c,
                           int32_t parts, const float* stat, float* dx, int64_t lddx, int32_t accumulate,
                           hypel_stream_t stream);
/* The same for `segs` row segments of `rows` rows each (the applications of a row-concatenated batch: every
 * application keeps its own whole-tensor norms); stat holds 2 floats per (segment, part), segment-major. */
int hypel_l2norm_segs_fwd(const float* x, int64_t ldx, int64_t rows, int32_t c, int32_t parts, int32_t segs, float* y,
                          int64_t ldy, float* stat, hypel_stream_t stream);
int hypel_l2norm_segs_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t rows, int32_t c,
                          int32_t parts, int32_t segs, const float* stat, float* dx, int64_t lddx, int32_t accumulate,
                          hypel_stream_t stream);
int hypel_l2norm_fwd(const float* x, int64_t ldx, int64_t rows, int32_t c, float* y, int64_t ldy, float* stat,
                     hypel_stream_t stream);
int hypel_l2norm_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t rows, int32_t c,
                     const float* stat, float* dx, int64_t lddx, int32_t accumulate, hypel_stream_t stream);
/* patch-NCE (cut_wrapper.py:360-420): g, r are [n][p][e] embeddings; per sample softmax-CE over the p*p logits
 * <g_a, r_b>/tau against the flattened identity; loss[0] (+)= weight * mean over n.  ws >= n + 1024 floats. */
int hypel_nce_loss(const float* g, int64_t ldg, const float* r, int64_t ldr, int64_t n, int32_t p, int32_t e,
                   float tau, float weight, float* loss, int32_t accumulate_loss, float* dg, int64_t lddg,
                   int32_t acc_dg, float* dr, int64_t lddr, int32_t acc_dr, float* ws, hypel_stream_t stream);

/* ---- capsule classifier (reference nnmodel/CAPModel.py; csrc/capsule.hip) -------------------------------------
 * Batch n, primary capsules i, classes j, capsule width d (<= HYPEL_CAPS_MAX_D), jd = j * d prediction columns
 * (<= HYPEL_CAPS_MAX_JD).  x[n][i][:] is a view of a pixel-major buffer: element pix[i / m] + n * ldx + (i % m) * d.
 * w is the [i][d][jd] slab of the per-capsule maps, bias [i][jd], uhat [n][i][jd].  All sums run in a fixed order inside
 * one block (no atomics): two runs give identical bits.
 *   uhat_fwd   uhat[n][i][:] = bias_i + x[n][i][:] . W_i                                     (reads W once)
 *   route_fwd  s[n][col] = sum_i coef[i][col / d] * uhat[n][i][col];  v = squash(s), q = mean(s^2) per capsule,
 *              v = q s / ((1 + q) sqrt(q + 1e-9));  y[n][j] = |v[n][j][:]| when y is not null
 *   agree_fwd  b_out[i][j] = b_in[i][j] (null = 0) + sum_n <uhat[n][i][j][:], v[n][j][:]>;  c_out = softmax_j(b_out);
 *              the routing logits b are fp64 buffers and both agree kernels sum in fp64 (b grows with the batch)
 *   head_bwd   dv = gy * v / |v| + gv (either may be null), ds = squash'(s) dv
 *   agree_bwd  dc[i][j] = sum_n <uhat[n][i][j][:], ds[n][j][:]>;  db = c * (dc - <c, dc>) + db_next (null = 0)
 *   route_bwd  dv[n][col] = sum_i coef[i][col / d] * uhat[n][i][col];  ds_out = squash'(s_in) dv
 *   uhat_bwd   duhat[n][i][col] = sum_t coefs[t][i][col / d] * vecs[t][n][col] (n_terms pairs, never stored);
 *              dw_i = x_i^T duhat_i, dbias_i = sum_n duhat_i (both or neither), dx[n][i][:] = duhat[n][i][:] . W_i^T
 *              at dpix[i / m] + n * lddx + (i % m) * d (null dx = skipped); acc_w / acc_x: add to what is there
 *   mask_fwd   out[n][e] = sum_j labels[n][j] * v[n][j * d + e];  mask_bwd: gv[n][j * d + e] (+)= labels[n][j] * gout[n][e]
 * Limits (a call outside them returns -1 before anything is launched): 1 <= n <= HYPEL_CAPS_MAX_N (the sample index is
 * a grid dimension), d <= HYPEL_CAPS_MAX_D, jd <= HYPEL_CAPS_MAX_JD, i % m == 0, jd % d == 0, and the dynamic LDS of the
 * two u_hat products <= HYPEL_CAPS_MAX_LDS bytes:
 *   uhat_fwd   4 * ((d + 1) * jd + 16 * d)
 *   uhat_bwd   4 * (d * jdp + 16 * jdp + 16 * d + n_terms * j),  jdp = jd | 1,  n_terms = 2 R - 1 for R routing iterations
 * At d = 16 the backward admits j <= 31 (and that only for R <= 4; j = 32 never), at d = 32 j <= 10; the forward alone
 * admits j = 32 at d = 16 and j <= 15 at d = 32.  hypelcnn_amd/graph.py::capsule_fits restates the rule and refuses such
 * a model when it is built. */
#define HYPEL_CAPS_MAX_D 32
#define HYPEL_CAPS_MAX_JD 512
#define HYPEL_CAPS_MAX_N 65535
#define HYPEL_CAPS_MAX_LDS 65536
int hypel_caps_uhat_fwd(const float* x, const int64_t* pix, int64_t ldx, int32_t m, const float* w, const float* bias,
                        int64_t n, int32_t i, int32_t d, int32_t jd, float* uhat, hypel_stream_t stream);
int hypel_caps_route_fwd(const float* uhat, const float* coef, int64_t n, int32_t i, int32_t j, int32_t d, float* s,
                         float* v, float* y, hypel_stream_t stream);
int hypel_caps_agree_fwd(const float* uhat, const float* v, int64_t n, int32_t i, int32_t j, int32_t d,
                         const double* b_in, double* b_out, float* c_out, hypel_stream_t stream);
int hypel_caps_head_bwd(const float* gy, const float* gv, const float* s, int64_t n, int32_t j, int32_t d, float* ds,
                        hypel_stream_t stream);
int hypel_caps_agree_bwd(const float* uhat, const float* ds, int64_t n, int32_t i, int32_t j, int32_t d, const float* c,
                         const float* db_next, float* db, hypel_stream_t stream);
int hypel_caps_route_bwd(const float* uhat, const float* coef, int64_t n, int32_t i, int32_t j, int32_t d,
                         const float* s_in, float* ds_out, hypel_stream_t stream);
int hypel_caps_uhat_bwd(const float* x, const int64_t* pix, int64_t ldx, int32_t m, const float* w, int64_t n, int32_t i,
                        int32_t j, int32_t d, int32_t n_terms, const float* coefs, const float* vecs, float* dw,
                        float* dbias, int32_t acc_w, float* dx, const int64_t* dpix, int64_t lddx, int32_t acc_x,
                        hypel_stream_t stream);
int hypel_caps_mask_fwd(const float* v, int64_t ldv, const float* labels, int64_t ldl, int64_t n, int32_t j, int32_t d,
                        float* out, int64_t ldo, hypel_stream_t stream);
int hypel_caps_mask_bwd(const float* gout, int64_t ldg, const float* labels, int64_t ldl, int64_t n, int32_t j, int32_t d,
                        float* gv, int64_t ldgv, int32_t accumulate, hypel_stream_t stream);

/* ---- kernel support-vector classifier (classify/classic_ml_trainer.py:46-54,105: sklearn.svm.SVC.fit / .predict, i.e.
 * libsvm's C-SVC with one-vs-one voting) ---------------------------------------------------------------------------
 * The two big products -- rows x vectors over the features, rows x pairs over the vectors -- are hypel_seg_gemm_f32
 * launches (HYPEL_GEMM_SPLIT6); these entry points are what sits between them.
 *
 * hypel_svm_center_norms_f32: x[r][0..cols) -= mean (mean NULL: left as it is), norms[r] = sum of squares of the row as
 *   stored afterwards, summed in fp64 (norms NULL: not written).  RBF only subtracts the training mean: distances do not
 *   change while |x|^2 falls by orders of magnitude, and one fp32 rounding of |x|^2 times gamma is the error of the
 *   exponent.  The polynomial kernel is not translation invariant and is never centred.
 * hypel_svm_kernel_apply_f32: inner products g[r][c] = x_r . z_c -> kernel values in place, one streaming pass.
 *   HYPEL_SVM_RBF: exp(-gamma max(0, row_norms[r] + col_norms[c] - 2 g)); HYPEL_SVM_POLY: (gamma g + coef0)^degree,
 *   degree 1..3.  Evaluated in fp64, stored fp32 (libsvm's Qfloat).
 * hypel_svm_smo_ovo: libsvm's Solver::Solve for C-SVC on every class pair at once, one workgroup per pair.  k is the
 *   whole training kernel matrix [l][ldk] with the rows sorted by class; pair p works on rows [a0, a0 + na) (y = +1,
 *   the lower class) and [b0, b0 + nb) (y = -1).  Second-order working-set selection (Fan, Chen, Lin 2005), clipped
 *   two-variable update, gradient update from two rows of k, stop when m(alpha) - M(alpha) < tol; no shrinking.
 *   alpha and the gradient are fp64 as in libsvm: in LDS while 3 * l_max doubles fit 48 KB, else in ws (3 doubles per
 *   element, pair p at ws + 3 * out_off; may be NULL when every pair fits).  Per pair: alpha_y[out_off + t] = alpha_t
 *   y_t, rho[p], obj[p] = the dual objective 1/2 a'Qa - sum a as the solver sees it, n_iter[p], status[p].  The loop is
 *   bounded: after max_iter (<= HYPEL_SVM_MAX_ITER_LIMIT) iterations a pair ends with HYPEL_SVM_NOT_CONVERGED and the
 *   caller raises.
 * hypel_svm_vote: dec[r][p] (pair order (0,1), (0,2) ... as svm_predict_values) -> label: dec > 0 votes for the lower
 *   class of the pair, anything else for the higher; the FIRST class with the maximal count wins.  The label is
 *   class_labels[winner] (NULL: the winner's index), written to out[y * raster_w + x] for points[r] = (x, y) -- the
 *   whole-scene path, like hypel_argmax_scatter -- or to out[r] when points is NULL.
 *
 * Grid search over (C, gamma) (ABI 8; hypelcnn_amd/classic/model_selection.py).  The inner products of a split do not
 * depend on gamma or C, every (gamma, C, class pair) problem is independent, and scoring stays on the device:
 * hypel_svm_kernel_planes_f32: g (read once, left intact) -> plane p at out + p * plane_stride, same ld, = what
 *   hypel_svm_kernel_apply_f32 writes in place for gammas[p] (a device array), bit for bit.  HYPEL_SVM_RBF only.
 * hypel_svm_smo_grid: hypel_svm_smo_ovo's solver (the same device function), one workgroup per job.  A job is a class
 *   pair (the hypel_svm_pair_t fields) on the plane of K at element offset k_off from k, with its own c.  Workgroup b
 *   solves job order[b] (order NULL: job b), so the issue order is the caller's while alpha_y[out_off ...], rho[j],
 *   obj[j], n_iter[j] and status[j] stay at the job's own index j; for the same K, pair, c, tol and max_iter they are
 *   bit-identical to hypel_svm_smo_ovo's.  Same bounded loop, same LDS / ws rule (job j at ws + 3 * out_off); a job
 *   at the cap ends with HYPEL_SVM_NOT_CONVERGED and stops nothing else.
 * hypel_svm_scatter_coef_f32: the n_c cells of one gamma (cell ci: alpha_y + ci * cell_stride, pair p at the pair
 *   table's out_off; rho[ci * n_pairs + p]) -> coef[l][n_c * npp] fp32 over ALL training rows, zero where a row is not
 *   in the pair or its multiplier is zero and in the pad columns p >= n_pairs, and bias[n_c * npp] = -rho.  The
 *   decisions of n_c cells are then one hypel_seg_gemm_f32: K_test plane [n_test][l] . coef + bias.
 * hypel_svm_vote_score: hypel_svm_vote's rule on every (row, cell) of dec[rows][n_cells * npp]; correct[cell] += the
 *   number of rows whose winner is truth[r] (class index; 2..255 classes).  Reduced in the block, one atomicAdd per block and cell;
 *   the caller zeroes correct.  No labels are written. */
enum { HYPEL_SVM_RBF = 0, HYPEL_SVM_POLY = 1 };
enum { HYPEL_SVM_CONVERGED = 0, HYPEL_SVM_NOT_CONVERGED = 1 };
#define HYPEL_SVM_MAX_ITER_LIMIT 1000000
typedef struct { int32_t a0; int32_t na; int32_t b0; int32_t nb; int64_t out_off; } hypel_svm_pair_t;
typedef struct { int32_t a0; int32_t na; int32_t b0; int32_t nb; int64_t out_off; int64_t k_off; double c; } hypel_svm_job_t;
int hypel_svm_center_norms_f32(float* x, int64_t ld, int64_t rows, int32_t cols, const float* mean, double* norms,
                               hypel_stream_t stream);
int hypel_svm_kernel_apply_f32(float* g, int64_t ld, int64_t rows, int32_t cols, int32_t kind, double gamma, double coef0,
                               int32_t degree, const double* row_norms, const double* col_norms, hypel_stream_t stream);
int hypel_svm_smo_ovo(const float* k, int64_t ldk, const hypel_svm_pair_t* pairs, int32_t n_pairs, int32_t l_max,
                      double c, double tol, int32_t max_iter, double* alpha_y, double* rho, double* obj, int32_t* n_iter,
                      int32_t* status, double* ws, hypel_stream_t stream);
int hypel_svm_vote(const float* dec, int64_t ld, int64_t rows, int32_t n_classes, const uint8_t* class_labels,
                   const int32_t* points, uint8_t* out, int64_t raster_w, hypel_stream_t stream);
int hypel_svm_kernel_planes_f32(const float* g, int64_t ld, int64_t rows, int32_t cols, int32_t kind, const double* gammas,
                                int32_t n_gamma, const double* row_norms, const double* col_norms, float* out,
                                int64_t plane_stride, hypel_stream_t stream);
int hypel_svm_smo_grid(const float* k, int64_t ldk, const hypel_svm_job_t* jobs, const int32_t* order, int32_t n_jobs,
                       int32_t l_max, double tol, int32_t max_iter, double* alpha_y, double* rho, double* obj,
                       int32_t* n_iter, int32_t* status, double* ws, hypel_stream_t stream);
int hypel_svm_scatter_coef_f32(const double* alpha_y, const double* rho, const hypel_svm_pair_t* pairs, int32_t n_pairs,
                               int32_t n_c, int64_t cell_stride, int32_t l, int32_t npp, float* coef, int64_t ldc,
                               float* bias, hypel_stream_t stream);
int hypel_svm_vote_score(const float* dec, int64_t ld, int64_t rows, int32_t n_classes, int32_t n_cells, int32_t npp,
                         const int32_t* truth, int32_t* correct, hypel_stream_t stream);

/* ---- scene preparation (BasicDataSet.__init__, common_nn_ops.py:45-72; AVONDataLoader's percentile clip) -------
 * The source raster is `src` + element strides: sample (y, x, b) of the [h, w, bands] scene is src[y*sy + x*sx + b*sb],
 * dtype HYPEL_DTYPE_* -- a transposed view of a file, or a window of its bands, is read in place.  Inputs are finite.
 *
 * hypel_scene_extrema: out_min[b] / out_max[b] (source dtype) = min / max over the scene of
 *   (T)(min(v, clip[b]) - sub[b]), computed in the source dtype (integers wrap); clip and sub are optional [bands]
 *   arrays of the source dtype.  ws: 2 * ws_slices * bands elements of the source dtype.
 * hypel_scene_rank_select_u16: out_lo[b] / out_hi[b] = the values at ranks rank_lo <= rank_hi (0-based, ascending) of
 *   band b's h*w samples, exactly.  ws: bands * HYPEL_SCENE_RANK_WS_WORDS uint32 (cleared by the call).
 * hypel_scene_prepare_f32: out [h+2*pad][w+2*pad][bands] float32 = float32((T)(min(v, clip[b]) - lo[b])) / scale[b]
 *   with v taken under numpy.pad(mode="symmetric") (any pad >= 0: the reflection has period 2h / 2w); clip, lo (source
 *   dtype) and scale (float32) are optional; the division is IEEE, correctly rounded (scale 0 gives NaN / inf).
 * hypel_scene_masked_sums: scene [hp][wp][bands] float32, map [hp][wp] uint8; sums[0*bands + b] = fp64 sum of band b
 *   over map != 0 (what calculate_shadow_ratio keeps as "in shadow"; for a 0 / 1 shadow map this is map == 1, for a
 *   map that marks shadow with another value, 255 say, only != 0 follows the reference), sums[1*bands + b] over
 *   map == 0; counts[2] the
 *   pixel counts.  One fixed summation order: two calls give identical bits.  ws: ws_slices * 2 * (bands + 1) doubles. */
#define HYPEL_SCENE_RANK_WS_WORDS 772
int hypel_scene_extrema(const void* src, int32_t dtype, int64_t h, int64_t w, int32_t bands, int64_t sy, int64_t sx,
                        int64_t sb, const void* clip, const void* sub, void* out_min, void* out_max, void* ws,
                        int32_t ws_slices, hypel_stream_t stream);
int hypel_scene_rank_select_u16(const uint16_t* src, int64_t h, int64_t w, int32_t bands, int64_t sy, int64_t sx,
                                int64_t sb, int64_t rank_lo, int64_t rank_hi, uint16_t* out_lo, uint16_t* out_hi,
                                uint32_t* ws, hypel_stream_t stream);
int hypel_scene_prepare_f32(const void* src, int32_t dtype, int64_t h, int64_t w, int32_t bands, int64_t sy, int64_t sx,
                            int64_t sb, int32_t pad, const void* clip, const void* lo, const float* scale, float* out,
                            hypel_stream_t stream);
int hypel_scene_masked_sums(const float* scene, const uint8_t* map, int64_t hp, int64_t wp, int32_t bands, double* sums,
                            int64_t* counts, double* ws, int32_t ws_slices, hypel_stream_t stream);

/* ---- band-ratio statistics (gan_common.py print_stats / create_stats; csrc/band_ratio.hip) -----------------------
 * hypel_band_ratio_f32: ratio[i*ld_ratio + b] = num[i*ld_num + b] / den[i*ld_den + b] * scale[b] for n rows of `bands`
 *   float32 (row strides in elements, each >= bands; scale optional: null = no multiplication).  The division is IEEE,
 *   correctly rounded, then the multiplication, rounded on its own: NumPy's float32 num / den * scale bit for bit.
 *   row_ok[i] (uint8) = 1 where every band of row i of the ratio is finite; *kept (device int64, cleared by the call) =
 *   the number of such rows.  Mask and count are integer work: two calls give identical bits.  1 <= n < 2^31.
 * hypel_column_rank_select_f32: out[r*bands + b] = the value at 0-based ascending rank ranks[r] of column b of
 *   x [n][bands] (float32, row stride ld) over the rows with row_ok[i] != 0 (null: all rows), exactly.  `kept` is the
 *   number of those rows (n when row_ok is null); `ranks` is a HOST array of n_ranks values in [0, kept), in any order,
 *   repeats allowed, 1 <= n_ranks <= HYPEL_COLUMN_RANK_MAX_RANKS -- all checked before anything is launched.  Rows
 *   masked out are never read and may hold NaN or inf; kept rows are finite.  Order is by value: -0.0 and +0.0 are
 *   equal and either may be returned.  ws: bands * HYPEL_COLUMN_RANK_WS_WORDS uint32, 16-byte aligned, cleared by the
 *   call.  Integer counts only: two calls give identical bits.  1 <= n < 2^31, bands <= HYPEL_COLUMN_RANK_MAX_BANDS. */
#define HYPEL_COLUMN_RANK_MAX_RANKS 8
#define HYPEL_COLUMN_RANK_MAX_BANDS 65536 /* columns of one hypel_column_rank_select_f32 call (a wider matrix: call per window) */
#define HYPEL_COLUMN_RANK_WS_WORDS 2320 /* 256 (level 1) + 8 * 256 (levels 2..4 per rank) + 8 * 2 (prefix, rank) */
int hypel_band_ratio_f32(const float* num, int64_t ld_num, const float* den, int64_t ld_den, int64_t n, int32_t bands,
                         const float* scale, float* ratio, int64_t ld_ratio, uint8_t* row_ok, int64_t* kept,
                         hypel_stream_t stream);
int hypel_column_rank_select_f32(const float* x, int64_t ld, int64_t n, int32_t bands, const uint8_t* row_ok,
                                 int64_t kept, const int64_t* ranks, int32_t n_ranks, float* out, uint32_t* ws,
                                 hypel_stream_t stream);

/* ---- TIFF layouts (common/tiff_io.py; csrc/tiff.hip) ---------------------------------------------------------------
 * From "the file's bytes are in HBM" to the raster [h][w][spp] the scene preparation reads.  A segment is a strip or
 * a tile; segment s of the table is plane s / (segs_across * segs_down) (chunky files have one plane), row of
 * segments (s / segs_across) % segs_down, column s % segs_across.  Offsets and lengths are bytes; the table lives in
 * device memory, so the caller checks it before upload (src ranges inside src, dst ranges inside dst and disjoint);
 * both launches still bound every read by src_len / src_bytes and every write by dst_len / dst_bytes.
 *
 * hypel_tiff_unpack: decodes segment s from src[src_off .. + src_len) to dst[dst_off .. + dst_len), one wavefront per
 *   segment, and writes status[s].  codec 5: TIFF LZW -- codes MSB-first, Clear 256, EOI 257, first free code 258,
 *   9 bits growing when the next free code reaches 511 / 1023 / 2047; decoding stops at EOI or once dst_len bytes
 *   exist.  codec 32773: PackBits -- header n in 0..127 copies n + 1 literals, -127..-1 repeats the next byte 1 - n
 *   times, -128 is a no-op; a run is clipped at dst_len.  A segment whose status is not HYPEL_TIFF_OK stops where the
 *   fault was met; nothing outside its dst range is written in any case.
 * hypel_tiff_assemble: out [h][w][spp] of `item`-byte samples in native order, chunky, from segments of
 *   seg_rows x seg_cols pixels (a strip: seg_cols = w) read at src + src_off (from_decoded 0: the file as it is) or
 *   src + dst_off (from_decoded 1: the buffer hypel_tiff_unpack or the host's inflate filled); planes 1 (chunky
 *   segments of spp samples per pixel) or spp (one sample per pixel, plane p feeds sample p).  Per segment row, over
 *   the full segment width: predictor 2 accumulates samples spp (chunky) or 1 (planar) apart, modulo the sample
 *   width, after the byte swap; predictor 3 (item 4) accumulates the row's bytes with that stride and re-interleaves
 *   its four byte planes, most significant first (swap is ignored: the planes have no byte order).  Right and bottom
 *   edge tiles and the short last strip are clipped.  A segment row that reaches past src_len / dst_len or src_bytes
 *   is left out. */
typedef struct {
    int64_t src_off, src_len; /* the segment in the file */
    int64_t dst_off, dst_len; /* its decoded bytes */
} hypel_tiff_seg_t;
enum { HYPEL_TIFF_LZW = 5, HYPEL_TIFF_PACKBITS = 32773 };
enum { HYPEL_TIFF_OK = 0, HYPEL_TIFF_BAD_CODE = 1, HYPEL_TIFF_BAD_FIRST = 2, HYPEL_TIFF_TRUNCATED = 3,
       HYPEL_TIFF_BAD_RANGE = 4 };
int hypel_tiff_unpack(const uint8_t* src, int64_t src_bytes, const hypel_tiff_seg_t* segs, int32_t n_segs,
                      int32_t codec, uint8_t* dst, int64_t dst_bytes, int32_t* status, hypel_stream_t stream);
int hypel_tiff_assemble(const uint8_t* src, int64_t src_bytes, const hypel_tiff_seg_t* segs, int32_t n_segs,
                        int32_t from_decoded, int64_t h, int64_t w, int32_t spp, int32_t item, int32_t seg_rows,
                        int32_t seg_cols, int32_t segs_across, int32_t planes, int32_t predictor, int32_t swap,
                        void* out, hypel_stream_t stream);

/* ---- shadow / lit pixel pairing (gan/gan_sampling_methods.py; csrc/pairs.hip) ---------------------------------------
 * What the samplers do to the shadow map, where the scene lives: the map is a uint8 [h][w] raster in HBM, the results
 * are the int32 [n][2] = (x, y) point lists hypel_gather_patches_f32 cuts the pairs from.  No atomics: two calls
 * write identical bytes.
 *
 * hypel_mask_dilate_l1_u8 replaces ndimage.binary_dilation(shadow_map, iterations=radius) (NeighborhoodBasedSampler,
 *   :29-30): out[y][x] = 1 where some pixel with map != 0 lies within L1 distance `radius` (>= 1) of (x, y), else 0;
 *   pixels outside the raster count as 0.  Two launches whatever the radius: a row pass leaves the horizontal distance
 *   to the nearest set pixel in ws (int32 [h][w]), a column pass takes min(|dy| + ws[y + dy][x]) <= radius.
 * hypel_pair_masks_u8 replaces the branch of the samplers' pixel loops (:41-46, :72-77): shadow[i] = map[i] == 1;
 *   lit[i] = map[i] != 1 when reach and margin are NULL (RandomBasedSampler), else
 *   reach[i] && !margin[i] && map[i] != 1 with reach / margin the dilations by neighborhood_size / margin (the ring the
 *   reference forms by a subtraction, visited by the `elif`); n = h * w.
 * hypel_mask_compact_points_i32 replaces the index bookkeeping of those loops (:36-46, :67-77): points[k] = (x, y) of
 *   the k-th pixel with mask != 0 in row-major scan order, for k < capacity (rows past `capacity` are not written);
 *   *count = the number of such pixels.  h * w < 2^31.  ws: ceil(h * w / HYPEL_COMPACT_TILE) int32.  Per-tile counts,
 *   a prefix sum over the tiles, then a scatter by ballot rank.
 * hypel_points_expand_i32 replaces numpy.repeat(..., repeats, axis=0) and the remainder vstack (RandomBasedSampler
 *   :80-82, TargetBasedSampler :171-175) on the point list: out[i] = points[i / repeat] for i < n * repeat, then
 *   out[n * repeat + j] = points[j] for j < remainder <= n.  repeat >= 0; n * repeat + remainder > 0. */
#define HYPEL_COMPACT_TILE 4096
int hypel_mask_dilate_l1_u8(const uint8_t* map, int64_t h, int64_t w, int32_t radius, uint8_t* out, int32_t* ws,
                            hypel_stream_t stream);
int hypel_pair_masks_u8(const uint8_t* map, const uint8_t* reach, const uint8_t* margin, int64_t n, uint8_t* shadow,
                        uint8_t* lit, hypel_stream_t stream);
int hypel_mask_compact_points_i32(const uint8_t* mask, int64_t h, int64_t w, int32_t* points, int64_t capacity,
                                  int32_t* count, int32_t* ws, hypel_stream_t stream);
int hypel_points_expand_i32(const int32_t* points, int64_t n, int32_t repeat, int64_t remainder, int32_t* out,
                            hypel_stream_t stream);

/* ---- shadow regions of a target image (utilities/reveal_shadow_targets.py; csrc/components.hip) ------------------
 * Rasters are [h][w] in row-major order, p = y * w + x; h * w < 2^31.  Integer work throughout: two calls write
 * identical bytes.
 *
 * hypel_components_label_u8: mask uint8, non-zero = inside.  root[p] (int32) = the row-major index of the first pixel
 *   of p's 8-connected component, -1 outside the mask.  Three launches: tiles of 64 x 16 pixels labelled in LDS, the
 *   links across tile borders merged (parent entries touched by device-scope atomics only; no block waits for
 *   another), every pixel walked to its root.  ws: h * w int32 (the parent table).  *status (device int32, cleared by
 *   the call) stays HYPEL_COMPONENTS_OK unless a walk ran into its step cap (4 * h * w + 64 per union, h * w per
 *   pixel of the last launch): then HYPEL_COMPONENTS_STEP_CAP is set, the walk is given up and root is not valid.
 * hypel_components_compact_i32: comp[p] (int32) = the rank of root[p] among all roots (root[r] == r) in row-major
 *   order, 0 .. n - 1, and -1 where root[p] is; *n_components (device int32) = n.  Per-tile counts, a prefix sum over
 *   the tiles, ranks by ballot -- no counter decides an id.  ws: ceil(h * w / HYPEL_COMPACT_TILE) int32.
 * hypel_components_votes_i32: targets uint8; votes [n_components][n_classes] int32 and size [n_components] int32 are
 *   cleared by the call.  size[c] = pixels with comp == c.  For every pixel p with comp[p] >= 0 and every one of its 8
 *   neighbours q inside the image with comp[q] < 0, targets[q] < n_classes and bit targets[q] of `exclude` clear:
 *   votes[comp[p]][targets[q]] += 1 (a lit pixel counts once for every component pixel it touches).  winner[c]
 *   (uint8) = the class with the most votes, the smallest such class on a tie, 255 where c has no vote.
 *   1 <= n_classes <= HYPEL_COMPONENTS_MAX_CLASSES; n_components = 0 launches nothing.
 * hypel_components_relabel_u8: out[p] = winner[comp[p]] where comp[p] >= 0 and that winner is not 255, else
 *   targets[p]; with plus_one != 0 every value other than 255 is then raised by 1.
 * hypel_shadow_correct_f32: out [h][w][bands] float32 = c + c * (m * r_minus_1[b]) with c = float32(sample (y, x, b))
 *   of the strided source (dtype HYPEL_DTYPE_*, element strides sy, sx, sb as in the scene preparation), m = 1.0f where
 *   map[y][x] != 0 and 0.0f elsewhere; both products and the sum are rounded on their own, in that order -- NumPy's
 *   float32 expression bit for bit (no fused multiply-add). */
#define HYPEL_COMPONENTS_MAX_CLASSES 64
enum { HYPEL_COMPONENTS_OK = 0, HYPEL_COMPONENTS_STEP_CAP = 1 };
int hypel_components_label_u8(const uint8_t* mask, int64_t h, int64_t w, int32_t* root, int32_t* ws, int32_t* status,
                              hypel_stream_t stream);
int hypel_components_compact_i32(const int32_t* root, int64_t h, int64_t w, int32_t* comp, int32_t* n_components,
                                 int32_t* ws, hypel_stream_t stream);
int hypel_components_votes_i32(const uint8_t* targets, const int32_t* comp, int64_t h, int64_t w, int32_t n_components,
                               int32_t n_classes, uint64_t exclude, int32_t* votes, int32_t* size, uint8_t* winner,
                               hypel_stream_t stream);
int hypel_components_relabel_u8(const uint8_t* targets, const int32_t* comp, const uint8_t* winner, int64_t h, int64_t w,
                                int32_t plus_one, uint8_t* out, hypel_stream_t stream);
int hypel_shadow_correct_f32(const void* src, int32_t dtype, int64_t h, int64_t w, int32_t bands, int64_t sy, int64_t sx,
                             int64_t sb, const uint8_t* map, const float* r_minus_1, float* out, hypel_stream_t stream);

/* ---- tensor summaries (tf.summary.histogram of the model variables; csrc/summary.hip) -------------------------------
 * hypel_tensor_summary_f32 summarises n_segs float32 tensors that are segments of ONE device buffer, where they live:
 * segment s is base[table[2s] ... table[2s] + table[2s + 1]) (int64 element offset >= 0 and size >= 0, any alignment,
 * any order, gaps allowed).  Per segment, with TensorFlow's histogram::Histogram::Add applied to every FINITE element
 * cast to double:
 *   stats[5s + 0..4] = min, max, num, sum, sum_squares (min / max start at +DBL_MAX / -DBL_MAX, num counts the finite
 *                      elements);
 *   nonfinite[s]     = the number of NaN / +-Inf elements, which take part in nothing else;
 *   buckets[s * n_limits + b] = the number of finite elements v with b = upper_bound(limits, v), the index of the first
 *                      limit strictly greater than v (clamped to n_limits - 1; TensorFlow's table ends in DBL_MAX).
 * limits: n_limits ascending doubles in device memory, 1 <= n_limits <= HYPEL_SUMMARY_MAX_LIMITS.  The bucket of an
 * element is estimated from its logarithm for TensorFlow's default table (1e-12 * 1.1^k, mirrored around 0.0) and then
 * corrected by comparisons against the table itself, so it is exact for ANY ascending table (slower for others).
 * Counts, min, max, num and nonfinite are exact.  sum / sum_squares are fp64 sums over a fixed partition (slices of
 * HYPEL_SUMMARY_SLICE elements, one block each) reduced in a fixed order, no floating-point atomics: two calls on the
 * same input give identical bits.
 * ws: HYPEL_SUMMARY_WS_DOUBLES(n_segs, ws_slices) doubles; ws_slices = the sum over the segments of
 * ceil(size / HYPEL_SUMMARY_SLICE), which the caller knows from the table it built.  A table that needs another
 * number of slices than ws_slices is refused on the device: every nonfinite[s] is then -1 and nothing else is valid. */
#define HYPEL_SUMMARY_SLICE 32768
#define HYPEL_SUMMARY_MAX_LIMITS 2048
#define HYPEL_SUMMARY_WS_DOUBLES(n_segs, ws_slices) ((int64_t)(n_segs) + 1 + 6 * (int64_t)(ws_slices))
int hypel_tensor_summary_f32(const float* base, const int64_t* table, int32_t n_segs, const double* limits,
                             int32_t n_limits, double* stats, int64_t* nonfinite, int64_t* buckets, double* ws,
                             int32_t ws_slices, hypel_stream_t stream);

/* ---- random forest of histogram trees (reference classify/classic_ml_trainer.py:46; csrc/forest.hip;
 * hypelcnn_amd/classic/forest.py) ---------------------------------------------------------------------------------------
 * Training rows are x [n][ld] float32 (finite), labels y int32 [n] in 0..n_classes-1, n_classes <=
 * HYPEL_FOREST_MAX_CLASSES (the LDS histogram [256][n_classes] int32 of hypel_forest_split_hist).  Every column is
 * quantised once; splits are searched over bin boundaries with integer class histograms.  Integer atomics only, every
 * choice among equals is a total order and every list is built by a prefix sum: two runs write identical bytes.
 *
 * hypel_forest_bin_edges_f32: one workgroup per column c < f.  With n_s = min(n, HYPEL_FOREST_EDGE_ROWS), the values
 *   x[perm[i]][c] + 0.0f, i < n_s, are sorted (perm: int32 [>= n_s], distinct rows in [0, n) -- beyond the cap a seeded
 *   subsample); for j = 1 .. n_bins-1 the value v at rank floor(j * n_s / n_bins) becomes an edge unless it equals the
 *   previous edge or the largest sampled value.  edges [f][HYPEL_FOREST_MAX_EDGES] ascending, unused slots +inf;
 *   n_edges [f].  2 <= n_bins <= 256.
 * hypel_forest_bin_u8: bins[c * ldn + i] = the number of edges of column c that are < x[i][c] (feature-major uint8,
 *   ldn >= n).  Hence bin <= t  <=>  x <= edges[c][t] for t < n_edges[c]: a grown node stores the raw float32 edge and
 *   is served by the rule x[feature] <= threshold.
 * Growth is level by level over all trees at once.  order (int32) holds, tree after tree, the tree's unique in-bag
 * rows; weight int32 [n_trees][n] their bootstrap multiplicity.  An active node is four int32: (tree, start, count,
 * node) = a segment order[start .. start + count) and the node's number.  cand int32 [n_active][max_features] are
 * the node's candidate columns, distinct per node (drawn on the host), 1 <= max_features <= f.
 * hypel_forest_split_hist: one workgroup per (active node a, slot s), record a * max_features + s: hist[bin][class] +=
 *   weight over the node's rows for column cand[a][s]; for every boundary t in 0..254 with both sides non-empty
 *   (weights nL, nR > 0; "left" = bin <= t)  score = (double)sum_k L_k^2 / (double)nL + (double)sum_k R_k^2 /
 *   (double)nR, the sums of squares exact in int64, each of the two divisions and the addition rounded once, no
 *   contraction.  Written: the largest score, its (lowest) bin, valid = 1; (0.0, -1, 0) when no boundary is valid or
 *   count < 2.
 * hypel_forest_split_apply: one workgroup per active node.  The best valid slot is the one with the largest score,
 *   then the lower column index, then the lower bin.  The node is a LEAF when count < 2, fewer than two classes have
 *   weight, no slot is valid, or level >= max_depth (<= HYPEL_FOREST_MAX_DEPTH); candidates are NOT redrawn when all
 *   are invalid (scikit-learn keeps drawing until it has seen every column).  Node record, at index `node`:
 *   feature (-1 leaf), thr_bin (-1), threshold = edges[feature][thr_bin] (0 for a leaf), left = right = -1 for a leaf,
 *   node_tree, node_count (unique rows), node_weight, value[node][n_classes] = class weight / node weight in fp64 (one
 *   division each).  A split node's segment is partitioned stably by bin <= thr_bin from order_in into order_out at the
 *   same positions (the two buffers alternate level by level; a leaf's segment is not copied).  Then, in active-node
 *   order, the r-th node that split gets left = node_base + 2r, right = left + 1 and the records (tree, start, nL,
 *   left), (tree, start + nL, count - nL, right) at next_active[2r], [2r + 1] (room for 2 * n_active records);
 *   counter[0] = 2 * (number of splits), which the host reads to size the next level, or -1 when a child's number
 *   would reach node_capacity (nothing is written past it: such a node keeps left = right = -1 and gets no records,
 *   the nodes that split before it keep theirs).  split_ws: int32 [n_active], left holding nL of a node that split
 *   and 0 of a leaf.  No node array is touched outside the records of the active nodes, no record of score, best_bin,
 *   valid or next_active outside the ones named here.
 * Extra-trees (reference classify/classic_ml_trainer.py:50, ExtraTreesClassifier): the same level-wise growth over the
 *   same operands -- y, weight, order, active, cand, the node arrays, split_ws, next_active and counter mean what they
 *   mean above -- but the split search reads the raw float32 values and never the bins: per record one random cut inside
 *   the node's range.
 * hypel_forest_columns_f32: xt[c * ldn + i] = x[i * ld + c] + 0.0f for i < n, c < f, ldn >= n: the feature-major float32
 *   copy with the sign of zero removed (so that a range does not depend on the order in which equal zeros are met).
 *   Elements i >= n of a row of xt are not written.
 * hypel_forest_split_random: one record per (active node a, slot s), at a * max_features + s, column c = cand[a][s];
 *   u float32 [n_active][max_features] in [0, 1) (drawn on the host).  Over the node's rows r = order[start .. start +
 *   count): lo = min xt[c][r], hi = max xt[c][r].  The record is valid when count >= 2 and lo < hi.  The cut is formed in
 *   float32, one rounding each, no contraction: d = hi - lo; m = u * d; t = lo + m; if (!(t < hi)) t = lo  (scikit-learn's
 *   own guard; it also catches d = inf of a column that spans more than the float32 range).  Hence lo <= t < hi and both
 *   sides hold a row, and weight: every row of a segment has weight >= 1 (order holds in-bag rows).  L_k = the weight
 *   of class k over the rows with xt[c][r] <= t, R_k the rest; score = (double)sum_k
 *   L_k^2 / (double)nL + (double)sum_k R_k^2 / (double)nR as in hypel_forest_split_hist: the sums of squares exact in
 *   int64, two divisions and one addition, each rounded once, no contraction.  Written: score, thr = t, valid = 1; or
 *   (0.0, 0.0f, 0).  No record of score, thr or valid outside n_active * max_features is touched.
 * hypel_forest_split_apply_thr: hypel_forest_split_apply with xt, ldn for bins, ldn and thr (float32, the table above) for
 *   best_bin and edges.  The best valid slot is the one with the largest score, then the lower column index (a node's
 *   columns are distinct: a total order).  Leaf reasons, node record, value, the compaction into next_active, counter
 *   (-1 at node_capacity included) and split_ws are exactly those of hypel_forest_split_apply, with two differences:
 *   threshold[node] = thr of the chosen slot (0 for a leaf) and thr_bin[node] = -1 always.  The stable partition goes by
 *   xt[feature][r] <= threshold, the float32 compare of the serving walk: every training row reaches the leaf it was
 *   counted in.  Integer atomics only, as above: two runs write identical bytes.
 * Serving: a model is one array of hypel_forest_node_t over all trees, 16-byte aligned (a record is one load; another
 *   alignment is refused) -- tree t's root is node tree_off[t] (int32 [n_trees]).  A node with left < 0 is a leaf and
 *   ends the walk at row -1 - left of leaf_value (fp64 [n_leaves][n_classes]); otherwise the walk goes to node `left` when x[feature] <= threshold (float32 compare) and to
 *   `right` if not; child indices are absolute and greater than their parent's (the walk is also bounded by n_nodes
 *   steps).  Per row the leaf rows are summed in tree order in fp64, divided by n_trees, and the FIRST maximum wins.
 *   The serving kernels do NOT check a model on the device: tree_off, child indices, leaf rows and feature values (a
 *   column < f, or a scene code inside the p x p window) are the caller's to validate, as ForestClassifier._set_model
 *   does on the host; a model that breaks them is read out of bounds.  The step bound limits the walk's length only.
 * hypel_forest_predict_rows: rows x [n][ld], feature < f.  The label, class_labels[winner] (NULL: the index), goes to
 *   out[i], or to out[y * raster_w + x] for points[i] = (x, y) like hypel_svm_vote; proba (optional) fp64
 *   [n][n_classes] receives the means.
 * hypel_forest_predict_scene: the same walk and vote for the p x p window with origin points[i] = (x, y) of the padded
 *   scene casi [hp][wp][cc], lidar [hp][wp][cl] (the arguments of hypel_gather_patches_f32), without cutting the
 *   patch: the feature field of scene_nodes[node] is 2 * e + a where a = 1 reads lidar and 0 casi, and e is the
 *   element offset from the window origin's pixel in that array -- (py * wp + px) * cc + ch for patch feature (py * p + px) * (cc + cl) + ch,
 *   ch < cc; (py * wp + px) * cl + ch - cc otherwise -- translated once when the model is uploaded.  The label goes
 *   to out[y * raster_w + x].
 * Diagnostics of a served model (scikit-learn's oob_decision_function_ / oob_score_, feature_importances_ and a grouped
 *   permutation importance).  The model arguments, the walk, the fp64 sum in tree order and the first maximum are those
 *   of hypel_forest_predict_rows; nothing below uses a floating-point atomic, so two runs write identical bytes.
 * hypel_forest_oob_rows: weight is an int32 table [n_trees][ldw] of bootstrap counts, ldw >= n.  Tree t does NOT vote
 *   for row i where weight[t * ldw + i] > 0.  votes[i] = the number of trees that vote; the leaf rows of the voting
 *   trees are summed in tree order in fp64 from 0.0 and each sum is divided once by (double)votes[i] into proba
 *   [n][n_classes]; out[i] = class_labels[first maximum] (NULL: the index).  A row no tree votes for has votes 0, a
 *   proba row of zeros and class index 0.  out, proba and votes are all required.  Rows are served in chunks by
 *   offsetting x, weight, proba, votes and out by the chunk's first row; ldw stays the table's row length.
 * hypel_forest_permuted_hits: column c belongs to group c % group_mod (group_mod >= 1; group_mod = f: every column its
 *   own group).  For every group g of [g0, g0 + n_groups) (inside [0, group_mod)), every repeat r < n_repeats and every
 *   row i, the walk reads x[partner[r * n + i]][c] for the columns c of group g and x[i][c] for the others; partner is
 *   int32 [n_repeats][n], each row a permutation of 0 .. n - 1.  Where the winner's class INDEX equals y[i] (int32 [n]),
 *   hits[(g - g0) * n_repeats + r] is incremented (integer atomics): the caller zeroes hits [n_groups][n_repeats], the
 *   launch adds to what it holds.  The grid is n_groups * n_repeats * ceil(n / 64) blocks; more than 2^31 - 1 are refused
 *   with a message that says so (launch fewer groups at a time).
 * hypel_forest_importances_f64: mean decrease in impurity.  nodes as for serving (children absolute, left < 0: a leaf),
 *   tree t owning the nodes tree_off[t] .. tree_off[t + 1] (n_nodes for the last tree), its root first; node_weight fp64
 *   [n_nodes] (the root's > 0); impurity fp64 [n_nodes], or NULL for Gini from value fp64 [n_nodes][n_classes] (every
 *   node's class fractions, not the leaf table): s = 0.0, s = s + v_k * v_k for k = 0 .. n_classes - 1 (product and
 *   addition rounded once each), impurity = 1.0 - s.  value and n_classes are read only when impurity is NULL.
 *   For an inner node j with children l, r: d = ((w_j * imp_j) - (w_l * imp_l)) - (w_r * imp_r), the three products and
 *   the two subtractions rounded once each, in this order.  raw[t][c] = the d of tree t's inner nodes with feature c,
 *   added one by one in ascending node order from 0.0.  Then, every step one rounding per element: raw[t][c] /= the
 *   weight of t's root; S_t = the sum of raw[t][0 .. f) in ascending column order from 0.0, and where S_t > 0,
 *   raw[t][c] /= S_t: that is per_tree [n_trees][f] (a lone root's row is zeros).  n_used[0] = the number of trees with
 *   more than one node.  importances[c] = (per_tree[t][c] of those trees, added in tree order from 0.0) / (double)n_used,
 *   then S = the sum of importances[0 .. f) in ascending column order from 0.0 and, where S > 0, importances[c] /= S.
 *   n_used = 0: importances is zeros.  (scikit-learn's arithmetic but for the two normalising sums, which numpy adds
 *   pairwise.)  The per-column sum runs in one workgroup per (tree, window of HYPEL_FOREST_IMPORTANCE_WINDOW columns)
 *   with an fp64 table and an int32 claim table in LDS: of a chunk of nodes, the lowest thread = node holding a decrease
 *   for a column claims the column, adds and retires, the others try again.  Like the serving kernels it does not
 *   validate the model. */
#define HYPEL_FOREST_EDGE_ROWS 16384
#define HYPEL_FOREST_IMPORTANCE_WINDOW 4096
#define HYPEL_FOREST_MAX_EDGES 255
#define HYPEL_FOREST_MAX_CLASSES 32
#define HYPEL_FOREST_MAX_DEPTH 64
typedef struct { int32_t feature; float threshold; int32_t left; int32_t right; } hypel_forest_node_t;
int hypel_forest_bin_edges_f32(const float* x, int64_t ld, int64_t n, int32_t f, const int32_t* perm, int32_t n_bins,
                               float* edges, int32_t* n_edges, hypel_stream_t stream);
int hypel_forest_bin_u8(const float* x, int64_t ld, int64_t n, int32_t f, const float* edges, const int32_t* n_edges,
                        uint8_t* bins, int64_t ldn, hypel_stream_t stream);
int hypel_forest_split_hist(const uint8_t* bins, int64_t ldn, const int32_t* y, const int32_t* weight, int64_t n,
                            int32_t n_classes, const int32_t* order, const int32_t* active, int32_t n_active,
                            const int32_t* cand, int32_t max_features, int32_t f, double* score, int32_t* best_bin,
                            int32_t* valid, hypel_stream_t stream);
int hypel_forest_split_apply(const uint8_t* bins, int64_t ldn, const int32_t* y, const int32_t* weight, int64_t n,
                             int32_t n_classes, const int32_t* order_in, int32_t* order_out, const int32_t* active,
                             int32_t n_active, const int32_t* cand, int32_t max_features, int32_t f, const double* score,
                             const int32_t* best_bin, const int32_t* valid, const float* edges, int32_t level,
                             int32_t max_depth, int32_t node_base, int32_t node_capacity, int32_t* feature,
                             int32_t* thr_bin, float* threshold, int32_t* left, int32_t* right, int32_t* node_tree,
                             int32_t* node_count, int32_t* node_weight, double* value, int32_t* split_ws,
                             int32_t* next_active, int32_t* counter, hypel_stream_t stream);
int hypel_forest_columns_f32(const float* x, int64_t ld, int64_t n, int32_t f, float* xt, int64_t ldn,
                             hypel_stream_t stream);
int hypel_forest_split_random(const float* xt, int64_t ldn, const int32_t* y, const int32_t* weight, int64_t n,
                              int32_t n_classes, const int32_t* order, const int32_t* active, int32_t n_active,
                              const int32_t* cand, const float* u, int32_t max_features, int32_t f, double* score,
                              float* thr, int32_t* valid, hypel_stream_t stream);
int hypel_forest_split_apply_thr(const float* xt, int64_t ldn, const int32_t* y, const int32_t* weight, int64_t n,
                                 int32_t n_classes, const int32_t* order_in, int32_t* order_out, const int32_t* active,
                                 int32_t n_active, const int32_t* cand, int32_t max_features, int32_t f,
                                 const double* score, const float* thr, const int32_t* valid, int32_t level,
                                 int32_t max_depth, int32_t node_base, int32_t node_capacity, int32_t* feature,
                                 int32_t* thr_bin, float* threshold, int32_t* left, int32_t* right, int32_t* node_tree,
                                 int32_t* node_count, int32_t* node_weight, double* value, int32_t* split_ws,
                                 int32_t* next_active, int32_t* counter, hypel_stream_t stream);
int hypel_forest_predict_rows(const float* x, int64_t ld, int64_t n, int32_t f, const int32_t* tree_off, int32_t n_trees,
                              const hypel_forest_node_t* nodes, int32_t n_nodes, const double* leaf_value,
                              int32_t n_leaves, int32_t n_classes, const uint8_t* class_labels, const int32_t* points,
                              uint8_t* out, int64_t raster_w, double* proba, hypel_stream_t stream);
int hypel_forest_predict_scene(const float* casi, const float* lidar, int64_t hp, int64_t wp, int32_t cc, int32_t cl,
                               const int32_t* points, int64_t n, int32_t p, const int32_t* tree_off, int32_t n_trees,
                               const hypel_forest_node_t* scene_nodes, int32_t n_nodes, const double* leaf_value,
                               int32_t n_leaves, int32_t n_classes, const uint8_t* class_labels, uint8_t* out,
                               int64_t raster_w, hypel_stream_t stream);
int hypel_forest_oob_rows(const float* x, int64_t ld, int64_t n, int32_t f, const int32_t* tree_off, int32_t n_trees,
                          const hypel_forest_node_t* nodes, int32_t n_nodes, const double* leaf_value, int32_t n_leaves,
                          int32_t n_classes, const uint8_t* class_labels, const int32_t* weight, int64_t ldw,
                          uint8_t* out, double* proba, int32_t* votes, hypel_stream_t stream);
int hypel_forest_permuted_hits(const float* x, int64_t ld, int64_t n, int32_t f, const int32_t* tree_off,
                               int32_t n_trees, const hypel_forest_node_t* nodes, int32_t n_nodes,
                               const double* leaf_value, int32_t n_leaves, int32_t n_classes, const int32_t* y,
                               const int32_t* partner, int32_t n_repeats, int32_t group_mod, int32_t g0,
                               int32_t n_groups, int32_t* hits, hypel_stream_t stream);
int hypel_forest_importances_f64(const hypel_forest_node_t* nodes, int32_t n_nodes, const int32_t* tree_off,
                                 int32_t n_trees, const double* value, int32_t n_classes, const double* node_weight,
                                 const double* impurity, int32_t f, double* per_tree, double* importances,
                                 int32_t* n_used, hypel_stream_t stream);

/* ---- template matching (utilities/lidar_matcher.py: cv2.resize INTER_AREA by an integer factor, cv2.matchTemplate
 * TM_CCORR_NORMED, cv2.minMaxLoc's max_loc; csrc/match.hip) ------------------------------------------------------------
 * A raster is ONE float32 band read in place: sample (y, x) of the [h][w] source is src[y*sy + x*sx] (element strides
 * >= 0; band b of a pixel-major [h][w][bands] scene is src + b with sx = bands), enlarged by pixel replication with the
 * integer factor scale >= 1: R'(Y, X) = R(Y / scale, X / scale), H = h * scale rows of W = w * scale columns.  The
 * enlarged raster is never written anywhere.  Image I' is H x W, template T' is HT x WT with HT <= H and WT <= W, the
 * output surface is hout x wout = (H - HT + 1) x (W - WT + 1), row-major; H * W, HT * WT and hout * wout are below
 * 2^31.  Inputs are finite (a NaN or an infinity anywhere is not supported: it spreads over every window it touches).
 *
 * hypel_match_ccorr_f32: num[y*wout + x] = sum_{i < HT, j < WT} T'(i, j) * I'(y + i, x + j) in float32 on the fp32
 *   matrix cores (v_mfma_f32_16x16x4_f32, an fmaf chain: every product exact, one rounding per addition).  HYPEL_MATCH_TILE
 *   output rows are the product of a Toeplitz band of one template column with a shifted window of the image,
 *   accumulated over the template's columns in chunks of HYPEL_MATCH_COL_CHUNK and over HYPEL_MATCH_TILE - 1 + HT image
 *   rows in chunks of HYPEL_MATCH_ROW_CHUNK; a block owns HYPEL_MATCH_TILE x HYPEL_MATCH_BLOCK_COLS outputs.  `splits`
 *   (1 .. HYPEL_MATCH_MAX_SPLITS) deals the (column chunk, row chunk) pairs, in that order, evenly to that many blocks
 *   per tile so that a surface of few tiles still fills the device: split s writes its partial surface to
 *   ws[s * hout * wout ...] and a second launch adds the partials in the order of s -- no float atomics, two calls
 *   give identical bits.  ws: splits * hout * wout float32, unused (may be null) when splits is 1;
 *   splits * hout * wout < 2^31.
 * hypel_match_window_energy_f64: energy[y*wout + x] = sum over the win_h x win_w window at (y, x) of R'^2 in double
 *   (a float32 squared is exact in double), hout x wout = (H - win_h + 1) x (W - win_w + 1).  Two separable passes:
 *   window sums along every SOURCE row into ws (h * wout doubles; a wavefront per 64 outputs: the first window summed
 *   by all lanes, the others by a prefix sum of what enters and what leaves), then down the columns (a thread per 32
 *   outputs: the first summed, the others slid).  At most 2 * (W + H) + 128 roundings per output, each relative to a
 *   partial sum of non-negative terms; a result the subtractions leave below zero (over a stretch of zeros) is stored
 *   as 0.  The window equal to the whole raster gives the template's energy as a 1 x 1 output.
 * hypel_match_best_f32: R = (float)((double)num / sqrt(energy * *e_t)), 0 where energy * *e_t == 0; division and square
 *   root are IEEE double.  score_map (optional) [hout * wout] float32 = R.  result: 16 bytes, 8-byte aligned -- float32
 *   best R at byte 0, zero at byte 4, int64 row-major index of it at byte 8; among equal values the smallest index (what
 *   cv2.minMaxLoc reports as max_loc = (index % wout, index / wout)).  The reduction is an integer atomic maximum of
 *   (R's bits in sortable order, ~index) and does not depend on the order of arrival.
 * hypel_match_render_u8: out [H][W] uint8 = (uint8)(R'(Y, X) / *max * 255), float32 division and product rounded on their
 *   own and truncated -- NumPy's (band / numpy.max(band) * 255).astype('uint8') for 0 <= band <= max; values outside
 *   0 .. 255 are clamped, *max <= 0 gives 0.  max: device float32 (hypel_scene_extrema of the band). */
#define HYPEL_MATCH_TILE 16
#define HYPEL_MATCH_ROW_CHUNK 32
#define HYPEL_MATCH_COL_CHUNK 32
#define HYPEL_MATCH_BLOCK_COLS 128
#define HYPEL_MATCH_MAX_SPLITS 4096
int hypel_match_ccorr_f32(const float* image, int64_t h, int64_t w, int64_t sy, int64_t sx, int32_t scale,
                          const float* tmpl, int64_t ht, int64_t wt, int64_t tsy, int64_t tsx, int32_t tscale, float* num,
                          float* ws, int32_t splits, hypel_stream_t stream);
int hypel_match_window_energy_f64(const float* src, int64_t h, int64_t w, int64_t sy, int64_t sx, int32_t scale,
                                  int64_t win_h, int64_t win_w, double* energy, double* ws, hypel_stream_t stream);
int hypel_match_best_f32(const float* num, const double* energy, const double* e_t, int64_t hout, int64_t wout,
                         float* score_map, void* result, hypel_stream_t stream);
int hypel_match_render_u8(const float* src, int64_t h, int64_t w, int64_t sy, int64_t sx, int32_t scale, const float* max,
                          uint8_t* out, hypel_stream_t stream);

/* ---- layer-activation range and histogram (utilities/nn_layer_activation_graph.py: numpy.histogram of the tapped
 * activations between their global minimum and maximum; common/device_activation.py, csrc/activation.hip) -------------
 * A VIEW is rows x cols float32 inside a row-major buffer with leading dimension ld >= cols: element (r, j) is
 * src[r * ld + j].  src is 4-byte aligned only (a tap's channel offset may be odd); what lies between the rows is never
 * read.  That is how a tap of a tower lies in its pixel-major plan buffer [npix][nb][ld]: one view of npix * nb rows at
 * its channel offset, or one view per run of consecutive pixels of a pixel map.  rows >= 0 (0: nothing is launched, the
 * outputs are untouched), cols >= 1, rows * cols < 2^37 (a block counts its share in 32 bits) and rows * ld <= 2^62;
 * anything else is refused.  Both calls ACCUMULATE into outputs the caller initialised, so that one tap is folded over
 * many batches and several views; the results are exact and independent of launch geometry and call order (integer
 * atomics only).
 *
 * hypel_view_range_f32: range[0] = min(range[0], v), range[1] = max(range[1], v) over the FINITE elements v (start them
 *   at +FLT_MAX / -FLT_MAX; a NaN or a -0.0 there is not supported), count[0] += the number of finite elements,
 *   count[1] += the number of NaN and +-Inf.  -0.0 counts as +0.0: which of the two a zero extreme comes back as is
 *   unspecified.  The extremes are integer atomics on the float's bits: signed order for v >= 0, reversed unsigned order
 *   for v < 0.
 * hypel_view_histogram_f32: edges is device float64 [n_bins + 1], strictly ascending, 1 <= n_bins <= HYPEL_ACT_MAX_BINS.
 *   A finite v with edges[0] <= v <= edges[n_bins] adds one to counts[k] for the k with edges[k] <= v < edges[k + 1], the
 *   last bin closed on the right (numpy.histogram on float64 data); a finite v outside adds one to outside[0]; NaN and
 *   +-Inf are counted nowhere.  The table decides the bin: it is estimated as (v - edges[0]) * n_bins / (edges[n_bins] -
 *   edges[0]) and corrected against the edges, held in LDS rounded up to float32 -- a few comparisons for a uniform
 *   table, a binary search for one that is far from it, exact for both.  One LDS histogram per block (8 * n_bins bytes of
 *   LDS), flushed once with 64-bit integer atomics on the non-zero counters. */
#define HYPEL_ACT_MAX_BINS 4096
int hypel_view_range_f32(const float* src, int64_t rows, int64_t ld, int32_t cols, float* range, int64_t* count,
                         hypel_stream_t stream);
int hypel_view_histogram_f32(const float* src, int64_t rows, int64_t ld, int32_t cols, const double* edges,
                             int32_t n_bins, int64_t* counts, int64_t* outside, hypel_stream_t stream);

/* ---- band PCA (classic/decomposition.py: BandPCA -- sklearn.decomposition.PCA over the band axis of a resident scene;
 * csrc/pca.hip) ----------------------------------------------------------------------------------------------------------
 * A VIEW is h rows of w pixels of c float32 bands with band stride 1: band b of pixel (y, x) is
 * x[y * stride_y + x * stride_x + b] (element strides >= c; the origin comes through the pointer, 4-byte aligned only).
 * That is the interior of a padded scene [hp][wp][C] (x = scene + n * (wp + 1) * C, stride_y = wp * C, stride_x = C) as
 * well as a plain row matrix (h = 1, stride_x = ld).  h, w >= 1, h * w <= 2^40, 1 <= c <= HYPEL_PCA_MAX_BANDS, strides
 * <= 2^40; anything else is refused, as are outputs or workspaces that overlap an input or each other.  Pixel p of a view
 * is (p / w, p % w); pixels are cut into chunks of HYPEL_PCA_CHUNK in that order.  No floating-point atomics anywhere:
 * partials go to a workspace and are added in a fixed order, so two calls on the same input give the same bits.
 *
 * hypel_pca_band_sums_f64: sums[b] = sum over the pixels of x_b in double (a float32 is exact in double; the error is
 *   that of n double additions).  Block g of G = min(chunks, HYPEL_PCA_MAX_BLOCKS) adds chunks g, g + G, ...; the G
 *   partials of a band are added by one block in a fixed order (strided shares, then a halving tree).  ws: G * c
 *   doubles, ws_doubles says how many there are.
 * hypel_pca_scatter_f64: scatter[i * c + j] = sum over the pixels of (x_i - mean_i) * (x_j - mean_j), the full symmetric
 *   [c][c] matrix (scatter[i][j] and scatter[j][i] are the same bits).  mean: device float32 [c].  Centred at load in
 *   float32 (one rounding per value); the products on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, an fmaf chain: every
 *   product exact, one rounding per addition); ONE float32 accumulator takes one chunk and no more, the chunk partials
 *   are added in double: in the order of the chunks inside a block, then in the order of the blocks.  The output is cut
 *   into tiles of HYPEL_PCA_TILE x HYPEL_PCA_TILE, T = nt * (nt + 1) / 2 of them on or above the diagonal (nt =
 *   ceil(c / HYPEL_PCA_TILE)); G = min(chunks, HYPEL_PCA_MAX_BLOCKS / T) blocks per tile.  ws: G * T * HYPEL_PCA_TILE^2
 *   doubles (at most HYPEL_PCA_MAX_BLOCKS * HYPEL_PCA_TILE^2 = 32 MiB), ws_doubles says how many there are.  A band
 *   that equals its mean in every pixel has a row and a column of exact zeros.
 * hypel_pca_project_f32: row r = pixel r of the view; out[r * ldo + j] = sum_b (x[r][b] - mean[b]) * weights[b * k + j]
 *   for j < k, and out[r * ldo + k + j] = x[r][c + j] for j < pass (trailing input floats of the pixel copied through, bit
 *   for bit; both strides >= c + pass).  weights: [c][k] row-major float32, 1 <= k <= c (whitening is folded into it by
 *   the host); ldo >= k + pass; columns of out beyond k + pass are not written.  Centred at load (not x W - mean W, which
 *   cancels); every output is ONE chain acc = fmaf(x_b - mean_b, W_bj, acc) over b = 0 .. c - 1 from 0, so the same
 *   pixel gives the same bits in any row, tail or grid pass.  A block owns 64 rows; at most
 *   HYPEL_PCA_PROJECT_MAX_BLOCKS blocks walk the rows.  The ranges of x and out must not overlap. */
#define HYPEL_PCA_MAX_BANDS 512
#define HYPEL_PCA_CHUNK 1024
#define HYPEL_PCA_TILE 64
#define HYPEL_PCA_MAX_BLOCKS 1024
#define HYPEL_PCA_PROJECT_MAX_BLOCKS 4096
int hypel_pca_band_sums_f64(const float* x, int64_t h, int64_t w, int32_t c, int64_t stride_y, int64_t stride_x,
                            double* sums, double* ws, int64_t ws_doubles, hypel_stream_t stream);
int hypel_pca_scatter_f64(const float* x, int64_t h, int64_t w, int32_t c, int64_t stride_y, int64_t stride_x,
                          const float* mean, double* scatter, double* ws, int64_t ws_doubles, hypel_stream_t stream);
int hypel_pca_project_f32(const float* x, int64_t h, int64_t w, int32_t c, int64_t stride_y, int64_t stride_x,
                          int32_t pass, const float* mean, const float* weights, int32_t k, float* out, int64_t ldo,
                          hypel_stream_t stream);

/* ---- grey-scale morphology (classic/morphology.py: MorphologicalProfile -- openings and closings by reconstruction of
 * a resident scene's channels, the extended morphological profile; csrc/morph.hip) ---------------------------------------
 * ORDER.  Every comparison is an unsigned compare of KEYS: a float32 with bit pattern u has the key
 * k = (u >> 31) ? ~u : (u | 0x80000000), and u = (k >> 31) ? (k & 0x7fffffff) : ~k gives it back exactly.  That is one
 * total order on all 2^32 patterns: -0 < +0, -inf below every finite value, +inf above, the NaNs at the two ends by
 * their sign bit.  All arithmetic is integer min / max on keys, every output is a bit copy of an input, nothing depends
 * on an evaluation order, and two calls on the same input give the same bits.  No floating-point atomics.
 * A key IMAGE is dense [h][w][c] uint32 (channel c of pixel (y, x) at (y * w + x) * c + ch); every channel is an
 * image of its own to the operators.  h, w >= 1, c >= 1, h, w < 2^31, h * w * c <= 2^40; anything else is refused, as
 * are null pointers and an output that overlaps an input.  A launch runs at most HYPEL_MORPH_MAX_BLOCKS blocks, each of
 * which walks (tile, channel) pairs or elements with the stride of the grid.
 *
 * hypel_morph_keys_u32: keys[(y * w + x) * c + ch] = key of x[y * stride_y + x * stride_x + ch] -- the VIEW of the band
 *   PCA above (element strides >= c, origin 4-byte aligned only), so the interior of a padded scene is read in place.
 * hypel_morph_erode_dilate_u32: dst = the minimum (op HYPEL_MORPH_ERODE) or maximum (HYPEL_MORPH_DILATE) of src over the
 *   structuring element of `radius` 0 .. HYPEL_MORPH_MAX_RADIUS: HYPEL_MORPH_DISK the offsets dx^2 + dy^2 <= radius^2
 *   (radius 1: the 4-neighbour cross), HYPEL_MORPH_SQUARE |dx|, |dy| <= radius; radius 0 copies.  Offsets outside the
 *   raster are ignored (erosion is padded with the largest key, dilation with the smallest); a radius larger than the
 *   raster is legal.  A block owns a tile of HYPEL_MORPH_TILE_W x HYPEL_MORPH_TILE_H pixels of one channel and holds
 *   it with its halo in LDS; the element is evaluated as one row span per dy.
 * hypel_morph_reconstruct_sweep_u32: one sweep of the reconstruction of `mask` from `marker_in`, by dilation (op
 *   HYPEL_MORPH_DILATE: the limit of m <- min(dilate3x3(m), mask) from m = min(marker, mask), 8-connectivity) or by erosion
 *   (HYPEL_MORPH_ERODE, the dual: max, erode3x3).  Per launch, for dilation (dual for erosion), pointwise:
 *   marker_out >= min(marker_in, mask); marker_out <= the limit; marker_out == marker_in exactly when marker_in is the
 *   limit; *changed is set to 1 exactly when they differ, and is never cleared.  A block iterates its tile (the same tile
 *   as above, one channel) to stability in LDS against the one-pixel halo of min(marker_in, mask) it loaded, so a launch
 *   carries a front across a tile, not a pixel.  marker_out must not overlap marker_in or mask (ping-pong buffers;
 *   marker_in and mask may be the same).
 * hypel_morph_profile_store_f32: the float32 of keys[y][x][b] goes to channel chan_offset + b * chan_step of the padded
 *   stack out [h + 2 pad][w + 2 pad][out_c], at (y + pad, x + pad) AND at every padding pixel that reflects onto (y, x)
 *   under numpy.pad(mode="symmetric") (index i < 0 reads -1 - i, i >= n reads 2 n - 1 - i): every padded pixel of the c
 *   channels is written once, no other channel of out is touched.  0 <= pad <= min(h, w) (one reflection), chan_step >= 1,
 *   chan_offset >= 0, chan_offset + (c - 1) * chan_step < out_c. */
#define HYPEL_MORPH_MAX_RADIUS 32
#define HYPEL_MORPH_MAX_BLOCKS 1024
#define HYPEL_MORPH_TILE_W 64
#define HYPEL_MORPH_TILE_H 16
enum { HYPEL_MORPH_DISK = 0, HYPEL_MORPH_SQUARE = 1 };
enum { HYPEL_MORPH_ERODE = 0, HYPEL_MORPH_DILATE = 1 };
int hypel_morph_keys_u32(const float* x, int64_t h, int64_t w, int32_t c, int64_t stride_y, int64_t stride_x,
                         uint32_t* keys, hypel_stream_t stream);
int hypel_morph_erode_dilate_u32(const uint32_t* src, int64_t h, int64_t w, int32_t c, int32_t radius, int32_t shape,
                                 int32_t op, uint32_t* dst, hypel_stream_t stream);
int hypel_morph_reconstruct_sweep_u32(const uint32_t* marker_in, const uint32_t* mask, int64_t h, int64_t w, int32_t c,
                                      int32_t op, uint32_t* marker_out, int32_t* changed, hypel_stream_t stream);
int hypel_morph_profile_store_f32(const uint32_t* keys, int64_t h, int64_t w, int32_t c, int32_t pad, float* out,
                                  int32_t out_c, int32_t chan_offset, int32_t chan_step, hypel_stream_t stream);

/* ---- graph capture helpers (HIP graphs instead of a tracing compiler) ---------------------------------------- */
int hypel_graph_begin_capture(hypel_stream_t stream);
int hypel_graph_end_capture(hypel_stream_t stream, void** graph_exec_out);
int hypel_graph_launch(void* graph_exec, hypel_stream_t stream);
int hypel_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* HYPEL_H */
