// Kernel support-vector classifier (include/hypel.h, hypel_svm_*): what sklearn.svm.SVC.fit / .predict do inside libsvm
// (reference classify/classic_ml_trainer.py:46-54,105).  The two big products of a fit and of a prediction (rows x
// vectors x features, rows x vectors x pairs) are hypel_seg_gemm_f32 launches; this file holds what sits between them:
//   center_norms   rows minus the training mean (RBF) and their squared norms, one pass
//   kernel_apply   inner products -> kernel values in place, one streaming pass
//   smo_ovo        libsvm's C-SVC SMO, one workgroup per class pair, all pairs in one launch
//   vote           pairwise decisions -> labels by libsvm's voting rule, scattered into a raster or written in order
// and the grid search over (C, gamma) (hypelcnn_amd/classic/model_selection.py):
//   kernel_planes  inner products -> one plane of kernel values per gamma, out of place, one pass
//   smo_grid       smo_ovo's solver on every (gamma, C, class pair) job of a chunk of the grid in one launch
//   scatter_coef   the multipliers of one gamma's jobs -> a dense coefficient matrix over all training rows
//   vote_score     vote's rule per (row, cell) -> the number of correct rows per cell
#include "common.h"
#include "wave.h"

namespace {

constexpr int SVM_THREADS = 256;
constexpr int SVM_WAVES = SVM_THREADS / 64;
constexpr double SVM_TAU = 1e-12;  // libsvm's floor of a non-positive curvature
constexpr int SVM_LDS_BYTES = 48 * 1024;

// ---- rows - mean, |row|^2 ------------------------------------------------------------------------------------------
// one wave per row; the sum of squares is taken over the values as STORED (after the fp32 subtraction), in fp64, so
// that |x|^2 + |z|^2 - 2 x.z is the distance of the stored rows to the rounding of the product alone
__global__ void __launch_bounds__(SVM_THREADS) svm_center_norms_kernel(float* __restrict__ x, int64_t ld, int64_t rows,
                                                                       int cols, const float* __restrict__ mean,
                                                                       double* __restrict__ norms) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * SVM_WAVES + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * SVM_WAVES;
    const bool vec = (ld & 3) == 0 && ((uintptr_t)x & 15) == 0 && (!mean || ((uintptr_t)mean & 15) == 0);
    for (int64_t r = wave0; r < rows; r += stride) {
        float* row = x + r * ld;
        double s = 0.0;
        if (vec) {
            const int quads = cols >> 2;
            for (int q = lane; q < quads; q += 64) {
                float4 v = reinterpret_cast<float4*>(row)[q];
                if (mean) {
                    const float4 m = reinterpret_cast<const float4*>(mean)[q];
                    v.x -= m.x, v.y -= m.y, v.z -= m.z, v.w -= m.w;
                    reinterpret_cast<float4*>(row)[q] = v;
                }
                s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
            }
            for (int c = (quads << 2) + lane; c < cols; c += 64) {
                float v = row[c];
                if (mean) row[c] = v = v - mean[c];
                s += (double)v * v;
            }
        } else {
            for (int c = lane; c < cols; c += 64) {
                float v = row[c];
                if (mean) row[c] = v = v - mean[c];
                s += (double)v * v;
            }
        }
        s = wave_sum(s);
        if (lane == 0 && norms) norms[r] = s;
    }
}

// ---- G -> K in place -----------------------------------------------------------------------------------------------
__device__ __forceinline__ float svm_kernel_value(float g, int kind, double gamma, double coef0, int degree, double rn,
                                                  double cn) {
    if (kind == HYPEL_SVM_RBF) {
        double d2 = rn + cn - 2.0 * (double)g;
        d2 = d2 > 0.0 ? d2 : 0.0;  // a distance: rounding may leave the self-product of a row a hair below zero
        return (float)exp(-gamma * d2);
    }
    const double b = gamma * (double)g + coef0;
    double v = b;
    if (degree >= 2) v *= b;
    if (degree >= 3) v *= b;
    return (float)v;
}

template <bool VEC>
__global__ void __launch_bounds__(SVM_THREADS) svm_kernel_apply_kernel(float* __restrict__ g, int64_t ld, int64_t rows,
                                                                       int cols, int kind, double gamma, double coef0,
                                                                       int degree, const double* __restrict__ rn,
                                                                       const double* __restrict__ cn) {
    const bool rbf = kind == HYPEL_SVM_RBF;
    if constexpr (VEC) {
        const int qpr = (cols + 3) >> 2;  // quads per row; ld % 4 == 0, so the last quad stays inside the row's pitch
        const int64_t total = rows * qpr;
        for (int64_t i = (int64_t)blockIdx.x * SVM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * SVM_THREADS) {
            const int64_t r = i / qpr;
            const int c = (int)(i - r * qpr) << 2;
            float4* p = reinterpret_cast<float4*>(g + r * ld + c);
            float4 v = *p;
            const double a = rbf ? rn[r] : 0.0;
            float* e = reinterpret_cast<float*>(&v);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < cols) e[k] = svm_kernel_value(e[k], kind, gamma, coef0, degree, a, rbf ? cn[c + k] : 0.0);
            *p = v;
        }
    } else {
        const int64_t total = rows * cols;
        for (int64_t i = (int64_t)blockIdx.x * SVM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * SVM_THREADS) {
            const int64_t r = i / cols;
            const int c = (int)(i - r * cols);
            float* p = g + r * ld + c;
            *p = svm_kernel_value(*p, kind, gamma, coef0, degree, rbf ? rn[r] : 0.0, rbf ? cn[c] : 0.0);
        }
    }
}

// ---- G -> n_gamma planes of K, out of place ---------------------------------------------------------------------------
// the grid search's form of kernel_apply: g is read once and left as it is, plane k = svm_kernel_value(g, gammas[k]).
// The distance is the same expression for every gamma, so the compiler evaluates it once per element.
template <bool VEC>
__global__ void __launch_bounds__(SVM_THREADS) svm_kernel_planes_kernel(const float* __restrict__ g, int64_t ld,
                                                                        int64_t rows, int cols,
                                                                        const double* __restrict__ gammas, int n_gamma,
                                                                        const double* __restrict__ rn,
                                                                        const double* __restrict__ cn,
                                                                        float* __restrict__ out, int64_t plane_stride) {
    if constexpr (VEC) {
        const int qpr = (cols + 3) >> 2;
        const int64_t total = rows * qpr;
        for (int64_t i = (int64_t)blockIdx.x * SVM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * SVM_THREADS) {
            const int64_t r = i / qpr;
            const int c = (int)(i - r * qpr) << 2;
            const int64_t at = r * ld + c;
            const float4 v = *reinterpret_cast<const float4*>(g + at);
            const float* e = reinterpret_cast<const float*>(&v);
            const double a = rn[r];
            double b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = c + k < cols ? cn[c + k] : 0.0;
            for (int p = 0; p < n_gamma; ++p) {
                const double gamma = gammas[p];
                float4 w = v;  // (pad columns of the last quad: g's own values, as kernel_apply leaves them)
                float* o = reinterpret_cast<float*>(&w);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < cols) o[k] = svm_kernel_value(e[k], HYPEL_SVM_RBF, gamma, 0.0, 0, a, b[k]);
                *reinterpret_cast<float4*>(out + p * plane_stride + at) = w;
            }
        }
    } else {
        const int64_t total = rows * cols;
        for (int64_t i = (int64_t)blockIdx.x * SVM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * SVM_THREADS) {
            const int64_t r = i / cols;
            const int c = (int)(i - r * cols);
            const float v = g[r * ld + c];
            const double a = rn[r], b = cn[c];
            for (int p = 0; p < n_gamma; ++p)
                out[p * plane_stride + r * ld + c] = svm_kernel_value(v, HYPEL_SVM_RBF, gammas[p], 0.0, 0, a, b);
        }
    }
}

// ---- SMO -----------------------------------------------------------------------------------------------------------
struct MaxIdx {
    double v;
    int i;
};
// maximum; among equal values the LARGER index (libsvm scans upwards with >=, so its last maximum wins)
__device__ __forceinline__ MaxIdx max_idx(MaxIdx a, MaxIdx b) {
    return (b.v > a.v || (b.v == a.v && b.i > a.i)) ? b : a;
}
__device__ __forceinline__ MaxIdx wave_down(MaxIdx m, int d) {  // (for wave_reduce)
    return MaxIdx{__shfl_down(m.v, d, 64), __shfl_down(m.i, d, 64)};
}
__device__ __forceinline__ MaxIdx wave_max_idx(MaxIdx m) {
    return wave_reduce(m, [](MaxIdx a, MaxIdx b) { return max_idx(a, b); });
}
__device__ __forceinline__ double wave_max(double v) {
    return wave_reduce(v, [](double a, double b) { return fmax(a, b); });
}

// One workgroup = one pair problem (hypel_svm_smo_ovo: one class pair of a fit; hypel_svm_smo_grid: one class pair of one
// (gamma, C) cell), solved by this one body so that the two entry points cannot drift.  Element t of the pair is row
// a0 + t of K (y = +1) for t < na, row b0 + t - na (y = -1) otherwise.  alpha / gradient / diagonal live in `alpha`
// (LDS or the caller's workspace, by the same pointer); element t is only ever touched by thread t % SVM_THREADS, except
// for the two-variable update by thread 0, which the barriers order.  Results go to alpha_y[pr.out_off ...] and to
// slot `out` of the per-problem arrays.
__device__ __forceinline__ void svm_smo_solve(const float* __restrict__ K, int64_t ldk, const hypel_svm_pair_t pr,
                                              double C, double tol, int max_iter, double* alpha,
                                              double* __restrict__ alpha_y, double* __restrict__ rho_out,
                                              double* __restrict__ obj_out, int32_t* __restrict__ iter_out,
                                              int32_t* __restrict__ status_out, int64_t out) {
    __shared__ MaxIdx part_a[SVM_WAVES];
    __shared__ MaxIdx part_b[SVM_WAVES];
    __shared__ double part_g2[SVM_WAVES];
    __shared__ double upd[2];
    __shared__ double fin[6][SVM_WAVES];

    const int na = pr.na, l = pr.na + pr.nb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* G = alpha + l;
    double* QD = G + l;
    auto row_of = [&](int t) -> int64_t { return t < na ? (int64_t)pr.a0 + t : (int64_t)pr.b0 + (t - na); };
    auto y_of = [&](int t) -> double { return t < na ? 1.0 : -1.0; };

    for (int t = tid; t < l; t += SVM_THREADS) {
        const int64_t r = row_of(t);
        alpha[t] = 0.0;
        G[t] = -1.0;
        QD[t] = (double)K[r * ldk + r];
    }
    __syncthreads();

    int iter = 0, status = HYPEL_SVM_NOT_CONVERGED;
    for (; iter < max_iter; ++iter) {
        // i: maximal violator of the "up" set
        MaxIdx m{-INFINITY, -1};
        for (int t = tid; t < l; t += SVM_THREADS) {
            const double a = alpha[t];
            const bool up = t < na ? a < C : a > 0.0;
            if (up) {
                const double v = t < na ? -G[t] : G[t];
                if (v >= m.v) m = MaxIdx{v, t};
            }
        }
        m = wave_max_idx(m);
        if (lane == 0) part_a[wave] = m;
        __syncthreads();  // A
        m = part_a[0];
#pragma unroll
        for (int w = 1; w < SVM_WAVES; ++w) m = max_idx(m, part_a[w]);
        const int i = m.i;
        const double gmax = m.v;
        if (i < 0) {  // empty up set: optimal
            status = HYPEL_SVM_CONVERGED;
            break;
        }
        const float* Ki = K + row_of(i) * ldk;
        const double qd_i = QD[i];
        // j: best second-order gain among the violators of the "low" set; Gmax2 for the stopping rule
        MaxIdx best{-INFINITY, -1};  // maximises -obj_diff = gain
        double g2 = -INFINITY;
        for (int t = tid; t < l; t += SVM_THREADS) {
            const double a = alpha[t];
            const bool low = t < na ? a > 0.0 : a < C;
            if (low) {
                const double yg = t < na ? G[t] : -G[t];
                g2 = fmax(g2, yg);
                const double gd = gmax + yg;
                if (gd > 0.0) {
                    double quad = qd_i + QD[t] - 2.0 * (double)Ki[row_of(t)];
                    if (!(quad > 0.0)) quad = SVM_TAU;
                    const double gain = gd * gd / quad;
                    if (gain >= best.v) best = MaxIdx{gain, t};
                }
            }
        }
        best = wave_max_idx(best);
        g2 = wave_max(g2);
        if (lane == 0) {
            part_b[wave] = best;
            part_g2[wave] = g2;
        }
        __syncthreads();  // B
        best = part_b[0];
        g2 = part_g2[0];
#pragma unroll
        for (int w = 1; w < SVM_WAVES; ++w) {
            best = max_idx(best, part_b[w]);
            g2 = fmax(g2, part_g2[w]);
        }
        const int j = best.i;
        if (gmax + g2 < tol || j < 0) {
            status = HYPEL_SVM_CONVERGED;
            break;
        }
        const float* Kj = K + row_of(j) * ldk;
        if (tid == 0) {  // libsvm's clipped two-variable update (Solver::Solve), C_i = C_j = C
            const double kij = (double)Ki[row_of(j)];
            double quad = qd_i + QD[j] - 2.0 * kij;
            if (!(quad > 0.0)) quad = SVM_TAU;
            const double ai0 = alpha[i], aj0 = alpha[j];
            double ai = ai0, aj = aj0;
            if ((i < na) != (j < na)) {
                const double delta = (-G[i] - G[j]) / quad;
                const double diff = ai - aj;
                ai += delta;
                aj += delta;
                if (diff > 0.0) {
                    if (aj < 0.0) aj = 0.0, ai = diff;
                } else {
                    if (ai < 0.0) ai = 0.0, aj = -diff;
                }
                if (diff > 0.0) {  // diff > C_i - C_j = 0
                    if (ai > C) ai = C, aj = C - diff;
                } else {
                    if (aj > C) aj = C, ai = C + diff;
                }
            } else {
                const double delta = (G[i] - G[j]) / quad;
                const double sum = ai + aj;
                ai -= delta;
                aj += delta;
                if (sum > C) {
                    if (ai > C) ai = C, aj = sum - C;
                } else {
                    if (aj < 0.0) aj = 0.0, ai = sum;
                }
                if (sum > C) {
                    if (aj > C) aj = C, ai = sum - C;
                } else {
                    if (ai < 0.0) ai = 0.0, aj = sum;
                }
            }
            alpha[i] = ai;
            alpha[j] = aj;
            upd[0] = (ai - ai0) * y_of(i);
            upd[1] = (aj - aj0) * y_of(j);
        }
        __syncthreads();  // C
        const double di = upd[0], dj = upd[1];
        for (int t = tid; t < l; t += SVM_THREADS) {
            const int64_t r = row_of(t);
            G[t] += y_of(t) * ((double)Ki[r] * di + (double)Kj[r] * dj);
        }
        // (no barrier: G[t] and alpha[t] belong to thread t % SVM_THREADS until thread 0 reads them behind A and B)
    }
    __syncthreads();

    // rho (Solver::calculate_rho), objective sum alpha (G - 1) / 2, alpha * y
    double ub = INFINITY, lb = -INFINITY, sum_free = 0.0, n_free = 0.0, obj = 0.0;
    for (int t = tid; t < l; t += SVM_THREADS) {
        const double a = alpha[t], y = y_of(t), yg = y * G[t];
        if (a >= C) {
            if (y < 0.0) ub = fmin(ub, yg);
            else lb = fmax(lb, yg);
        } else if (a <= 0.0) {
            if (y > 0.0) ub = fmin(ub, yg);
            else lb = fmax(lb, yg);
        } else {
            n_free += 1.0;
            sum_free += yg;
        }
        obj += a * (G[t] - 1.0);
        alpha_y[pr.out_off + t] = a * y;
    }
    ub = -wave_max(-ub);
    lb = wave_max(lb);
    sum_free = wave_sum(sum_free);
    n_free = wave_sum(n_free);
    obj = wave_sum(obj);
    if (lane == 0) {
        fin[0][wave] = ub, fin[1][wave] = lb, fin[2][wave] = sum_free, fin[3][wave] = n_free, fin[4][wave] = obj;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SVM_WAVES; ++w) {
            ub = fmin(ub, fin[0][w]);
            lb = fmax(lb, fin[1][w]);
            sum_free += fin[2][w];
            n_free += fin[3][w];
            obj += fin[4][w];
        }
        rho_out[out] = n_free > 0.0 ? sum_free / n_free : (ub + lb) / 2.0;
        obj_out[out] = obj / 2.0;
        iter_out[out] = iter;
        status_out[out] = status;
    }
}

__global__ void __launch_bounds__(SVM_THREADS) svm_smo_ovo_kernel(const float* __restrict__ K, int64_t ldk,
                                                                  const hypel_svm_pair_t* __restrict__ pairs, double C,
                                                                  double tol, int max_iter, double* __restrict__ alpha_y,
                                                                  double* __restrict__ rho_out, double* __restrict__ obj_out,
                                                                  int32_t* __restrict__ iter_out,
                                                                  int32_t* __restrict__ status_out, double* __restrict__ ws,
                                                                  int use_lds) {
    extern __shared__ double svm_lds[];
    const hypel_svm_pair_t pr = pairs[blockIdx.x];
    svm_smo_solve(K, ldk, pr, C, tol, max_iter, use_lds ? svm_lds : ws + 3 * pr.out_off, alpha_y, rho_out, obj_out,
                  iter_out, status_out, blockIdx.x);
}

// The grid search's launch: block b solves job order[b] (order NULL: job b) -- a pair of one (gamma, C) cell on that
// gamma's plane of K, with that cell's C.  A job that reaches the cap ends NOT_CONVERGED like a pair of smo_ovo; nothing
// a job does can stop another.
__global__ void __launch_bounds__(SVM_THREADS) svm_smo_grid_kernel(const float* __restrict__ K, int64_t ldk,
                                                                   const hypel_svm_job_t* __restrict__ jobs,
                                                                   const int32_t* __restrict__ order, double tol,
                                                                   int max_iter, double* __restrict__ alpha_y,
                                                                   double* __restrict__ rho_out, double* __restrict__ obj_out,
                                                                   int32_t* __restrict__ iter_out,
                                                                   int32_t* __restrict__ status_out, double* __restrict__ ws,
                                                                   int use_lds) {
    extern __shared__ double svm_lds[];
    const int64_t j = order ? order[blockIdx.x] : (int64_t)blockIdx.x;
    const hypel_svm_job_t jb = jobs[j];
    const hypel_svm_pair_t pr{jb.a0, jb.na, jb.b0, jb.nb, jb.out_off};
    svm_smo_solve(K + jb.k_off, ldk, pr, jb.c, tol, max_iter, use_lds ? svm_lds : ws + 3 * jb.out_off, alpha_y, rho_out,
                  obj_out, iter_out, status_out, j);
}

// ---- votes ---------------------------------------------------------------------------------------------------------
// one thread per row; the vote counters (at most n_classes - 1 <= 255 each) sit in LDS as bytes, class-major so that
// the threads of a wave hit consecutive banks
__global__ void __launch_bounds__(SVM_THREADS) svm_vote_kernel(const float* __restrict__ dec, int64_t ld, int64_t rows,
                                                               int n_classes, const uint8_t* __restrict__ class_labels,
                                                               const int32_t* __restrict__ points,
                                                               uint8_t* __restrict__ out, int64_t raster_w) {
    extern __shared__ uint8_t votes[];
    const int tid = threadIdx.x;
    for (int64_t r0 = (int64_t)blockIdx.x * SVM_THREADS; r0 < rows; r0 += (int64_t)gridDim.x * SVM_THREADS) {
        const int64_t r = r0 + tid;
        if (r >= rows) continue;  // (no barrier below: a thread reads only its own counters)
        for (int c = 0; c < n_classes; ++c) votes[c * SVM_THREADS + tid] = 0;
        const float* d = dec + r * ld;
        int p = 0;
        for (int a = 0; a < n_classes; ++a)
            for (int b = a + 1; b < n_classes; ++b, ++p) {
                const int w = d[p] > 0.0f ? a : b;  // libsvm svm_predict_values: dec > 0 -> the lower class
                votes[w * SVM_THREADS + tid] += 1;
            }
        int best = 0, best_n = votes[tid];
        for (int c = 1; c < n_classes; ++c) {
            const int n = votes[c * SVM_THREADS + tid];
            if (n > best_n) best_n = n, best = c;  // first class with the maximal count
        }
        const uint8_t label = class_labels ? class_labels[best] : (uint8_t)best;
        if (points) out[(int64_t)points[2 * r + 1] * raster_w + points[2 * r]] = label;
        else out[r] = label;
    }
}

// ---- grid search: multipliers -> dense coefficients, decisions -> correct rows per cell -----------------------------------
// coef[r][ci * npp + p] = alpha_y of training row r in pair p of cell ci (0 where r is in neither class of the pair, and
// in the pad columns p >= n_pairs); bias = -rho.  Every element of both outputs is written: no pre-zeroing.
__global__ void __launch_bounds__(SVM_THREADS) svm_scatter_coef_kernel(const double* __restrict__ alpha_y,
                                                                       const double* __restrict__ rho,
                                                                       const hypel_svm_pair_t* __restrict__ pairs,
                                                                       int n_pairs, int n_c, int64_t cell_stride, int l,
                                                                       int npp, float* __restrict__ coef, int64_t ldc,
                                                                       float* __restrict__ bias) {
    const int n_cols = n_c * npp;
    const int64_t total = (int64_t)l * n_cols;
    const int64_t first = (int64_t)blockIdx.x * SVM_THREADS + threadIdx.x, step = (int64_t)gridDim.x * SVM_THREADS;
    for (int64_t i = first; i < total; i += step) {
        const int r = (int)(i / n_cols);
        const int col = (int)(i - (int64_t)r * n_cols);
        const int ci = col / npp, p = col - ci * npp;
        float v = 0.0f;
        if (p < n_pairs) {
            const hypel_svm_pair_t pr = pairs[p];
            const double* ay = alpha_y + ci * cell_stride + pr.out_off;
            if (r >= pr.a0 && r < pr.a0 + pr.na) v = (float)ay[r - pr.a0];
            else if (r >= pr.b0 && r < pr.b0 + pr.nb) v = (float)ay[pr.na + (r - pr.b0)];
        }
        coef[(int64_t)r * ldc + col] = v;
    }
    for (int64_t col = first; col < n_cols; col += step) {
        const int ci = (int)col / npp, p = (int)col - ci * npp;
        bias[col] = p < n_pairs ? (float)-rho[(int64_t)ci * n_pairs + p] : 0.0f;
    }
}

// svm_vote_kernel's rule on cell blockIdx.y of dec[rows][n_cells * npp]; the rows whose winner is truth[r] are counted in
// the block (wave shuffle, then LDS) and reach correct[cell] as one atomicAdd per block and cell
__global__ void __launch_bounds__(SVM_THREADS) svm_vote_score_kernel(const float* __restrict__ dec, int64_t ld,
                                                                     int64_t rows, int n_classes, int npp,
                                                                     const int32_t* __restrict__ truth,
                                                                     int32_t* __restrict__ correct) {
    extern __shared__ uint8_t votes[];
    __shared__ int part[SVM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cell = blockIdx.y;
    int hit = 0;
    for (int64_t r0 = (int64_t)blockIdx.x * SVM_THREADS; r0 < rows; r0 += (int64_t)gridDim.x * SVM_THREADS) {
        const int64_t r = r0 + tid;
        if (r < rows) {  // (a thread reads only its own counters: no barrier inside)
            for (int c = 0; c < n_classes; ++c) votes[c * SVM_THREADS + tid] = 0;
            const float* d = dec + r * ld + (int64_t)cell * npp;
            int p = 0;
            for (int a = 0; a < n_classes; ++a)
                for (int b = a + 1; b < n_classes; ++b, ++p) {
                    const int w = d[p] > 0.0f ? a : b;
                    votes[w * SVM_THREADS + tid] += 1;
                }
            int best = 0, best_n = votes[tid];
            for (int c = 1; c < n_classes; ++c) {
                const int n = votes[c * SVM_THREADS + tid];
                if (n > best_n) best_n = n, best = c;
            }
            hit += best == truth[r];
        }
    }
    hit = wave_sum(hit);
    if (lane == 0) part[wave] = hit;
    __syncthreads();
    if (tid == 0) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < SVM_WAVES; ++w) n += part[w];
        if (n) atomicAdd(correct + cell, n);
    }
}

}  // namespace

extern "C" int hypel_svm_center_norms_f32(float* x, int64_t ld, int64_t rows, int32_t cols, const float* mean,
                                          double* norms, hypel_stream_t stream) {
    HYPEL_REQUIRE(x && rows >= 0 && cols > 0 && ld >= cols && (mean || norms), "hypel_svm_center_norms_f32");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(svm_center_norms_kernel, dim3(hypel_grid_1d(rows, SVM_WAVES)), dim3(SVM_THREADS), 0,
                       (hipStream_t)stream, x, ld, rows, cols, mean, norms);
    HYPEL_CHECK_LAUNCH("hypel_svm_center_norms_f32");
    return 0;
}

extern "C" int hypel_svm_kernel_apply_f32(float* g, int64_t ld, int64_t rows, int32_t cols, int32_t kind, double gamma,
                                          double coef0, int32_t degree, const double* row_norms, const double* col_norms,
                                          hypel_stream_t stream) {
    HYPEL_REQUIRE(g && rows >= 0 && cols > 0 && ld >= cols, "hypel_svm_kernel_apply_f32");
    HYPEL_REQUIRE(kind == HYPEL_SVM_RBF || kind == HYPEL_SVM_POLY, "hypel_svm_kernel_apply_f32: kernel is rbf or poly");
    HYPEL_REQUIRE(kind != HYPEL_SVM_RBF || (row_norms && col_norms), "hypel_svm_kernel_apply_f32: rbf needs both norms");
    HYPEL_REQUIRE(kind != HYPEL_SVM_POLY || (degree >= 1 && degree <= 3), "hypel_svm_kernel_apply_f32: degree is 1..3");
    if (rows == 0) return 0;
    const bool vec = (ld & 3) == 0 && ((uintptr_t)g & 15) == 0;
    const int64_t items = vec ? rows * ((cols + 3) / 4) : rows * (int64_t)cols;
    const int grid = hypel_grid_1d(items, SVM_THREADS);
    if (vec)
        hipLaunchKernelGGL(svm_kernel_apply_kernel<true>, dim3(grid), dim3(SVM_THREADS), 0, (hipStream_t)stream, g, ld, rows,
                           cols, kind, gamma, coef0, degree, row_norms, col_norms);
    else
        hipLaunchKernelGGL(svm_kernel_apply_kernel<false>, dim3(grid), dim3(SVM_THREADS), 0, (hipStream_t)stream, g, ld,
                           rows, cols, kind, gamma, coef0, degree, row_norms, col_norms);
    HYPEL_CHECK_LAUNCH("hypel_svm_kernel_apply_f32");
    return 0;
}

extern "C" int hypel_svm_smo_ovo(const float* k, int64_t ldk, const hypel_svm_pair_t* pairs, int32_t n_pairs,
                                 int32_t l_max, double c, double tol, int32_t max_iter, double* alpha_y, double* rho,
                                 double* obj, int32_t* n_iter, int32_t* status, double* ws, hypel_stream_t stream) {
    HYPEL_REQUIRE(k && pairs && alpha_y && rho && obj && n_iter && status, "hypel_svm_smo_ovo");
    HYPEL_REQUIRE(n_pairs >= 0 && l_max > 0 && ldk > 0 && c > 0.0 && tol > 0.0, "hypel_svm_smo_ovo");
    HYPEL_REQUIRE(max_iter > 0 && max_iter <= HYPEL_SVM_MAX_ITER_LIMIT,
                  "hypel_svm_smo_ovo: the iteration cap is bounded (a solver must not spin on a shared device)");
    if (n_pairs == 0) return 0;
    const size_t need = (size_t)3 * l_max * sizeof(double);
    const int use_lds = need <= (size_t)SVM_LDS_BYTES;
    HYPEL_REQUIRE(use_lds || ws, "hypel_svm_smo_ovo: a pair beyond the LDS budget needs the workspace");
    hipLaunchKernelGGL(svm_smo_ovo_kernel, dim3(n_pairs), dim3(SVM_THREADS), use_lds ? need : 0, (hipStream_t)stream, k, ldk,
                       pairs, c, tol, max_iter, alpha_y, rho, obj, n_iter, status, ws, use_lds);
    HYPEL_CHECK_LAUNCH("hypel_svm_smo_ovo");
    return 0;
}

extern "C" int hypel_svm_vote(const float* dec, int64_t ld, int64_t rows, int32_t n_classes, const uint8_t* class_labels,
                              const int32_t* points, uint8_t* out, int64_t raster_w, hypel_stream_t stream) {
    HYPEL_REQUIRE(dec && out && rows >= 0, "hypel_svm_vote");
    HYPEL_REQUIRE(n_classes >= 2 && n_classes <= 256, "hypel_svm_vote: 2..256 classes (uint8 labels)");
    HYPEL_REQUIRE(ld >= (int64_t)n_classes * (n_classes - 1) / 2, "hypel_svm_vote: ld < number of pairs");
    HYPEL_REQUIRE(!points || raster_w > 0, "hypel_svm_vote");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(svm_vote_kernel, dim3(hypel_grid_1d(rows, SVM_THREADS)), dim3(SVM_THREADS),
                       (size_t)n_classes * SVM_THREADS, (hipStream_t)stream, dec, ld, rows, n_classes, class_labels, points,
                       out, raster_w);
    HYPEL_CHECK_LAUNCH("hypel_svm_vote");
    return 0;
}

extern "C" int hypel_svm_kernel_planes_f32(const float* g, int64_t ld, int64_t rows, int32_t cols, int32_t kind,
                                           const double* gammas, int32_t n_gamma, const double* row_norms,
                                           const double* col_norms, float* out, int64_t plane_stride,
                                           hypel_stream_t stream) {
    HYPEL_REQUIRE(kind == HYPEL_SVM_RBF, "hypel_svm_kernel_planes_f32: rbf only (the grid search is over SVC(), whose "
                                         "kernel is rbf; poly is hypel_svm_kernel_apply_f32's)");
    HYPEL_REQUIRE(g && out && gammas && row_norms && col_norms && rows >= 0 && cols > 0 && ld >= cols && n_gamma > 0,
                  "hypel_svm_kernel_planes_f32");
    HYPEL_REQUIRE(plane_stride >= rows * ld, "hypel_svm_kernel_planes_f32: planes overlap");
    const float* g_end = g + rows * ld;
    const float* o_end = out + (n_gamma - 1) * plane_stride + rows * ld;
    HYPEL_REQUIRE(o_end <= g || g_end <= out, "hypel_svm_kernel_planes_f32: out of place (g is left intact)");
    if (rows == 0) return 0;
    const bool vec = (ld & 3) == 0 && (plane_stride & 3) == 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const int64_t items = vec ? rows * ((cols + 3) / 4) : rows * (int64_t)cols;
    const int grid = hypel_grid_1d(items, SVM_THREADS);
    if (vec)
        hipLaunchKernelGGL(svm_kernel_planes_kernel<true>, dim3(grid), dim3(SVM_THREADS), 0, (hipStream_t)stream, g, ld, rows,
                           cols, gammas, n_gamma, row_norms, col_norms, out, plane_stride);
    else
        hipLaunchKernelGGL(svm_kernel_planes_kernel<false>, dim3(grid), dim3(SVM_THREADS), 0, (hipStream_t)stream, g, ld,
                           rows, cols, gammas, n_gamma, row_norms, col_norms, out, plane_stride);
    HYPEL_CHECK_LAUNCH("hypel_svm_kernel_planes_f32");
    return 0;
}

extern "C" int hypel_svm_smo_grid(const float* k, int64_t ldk, const hypel_svm_job_t* jobs, const int32_t* order,
                                  int32_t n_jobs, int32_t l_max, double tol, int32_t max_iter, double* alpha_y, double* rho,
                                  double* obj, int32_t* n_iter, int32_t* status, double* ws, hypel_stream_t stream) {
    HYPEL_REQUIRE(k && jobs && alpha_y && rho && obj && n_iter && status, "hypel_svm_smo_grid");
    HYPEL_REQUIRE(n_jobs >= 0 && l_max > 0 && ldk > 0 && tol > 0.0, "hypel_svm_smo_grid");
    HYPEL_REQUIRE(max_iter > 0 && max_iter <= HYPEL_SVM_MAX_ITER_LIMIT,
                  "hypel_svm_smo_grid: the iteration cap is bounded (a solver must not spin on a shared device)");
    if (n_jobs == 0) return 0;
    const size_t need = (size_t)3 * l_max * sizeof(double);
    const int use_lds = need <= (size_t)SVM_LDS_BYTES;
    HYPEL_REQUIRE(use_lds || ws, "hypel_svm_smo_grid: a pair beyond the LDS budget needs the workspace");
    hipLaunchKernelGGL(svm_smo_grid_kernel, dim3(n_jobs), dim3(SVM_THREADS), use_lds ? need : 0, (hipStream_t)stream, k, ldk,
                       jobs, order, tol, max_iter, alpha_y, rho, obj, n_iter, status, ws, use_lds);
    HYPEL_CHECK_LAUNCH("hypel_svm_smo_grid");
    return 0;
}

extern "C" int hypel_svm_scatter_coef_f32(const double* alpha_y, const double* rho, const hypel_svm_pair_t* pairs,
                                          int32_t n_pairs, int32_t n_c, int64_t cell_stride, int32_t l, int32_t npp,
                                          float* coef, int64_t ldc, float* bias, hypel_stream_t stream) {
    HYPEL_REQUIRE(alpha_y && rho && pairs && coef && bias, "hypel_svm_scatter_coef_f32");
    HYPEL_REQUIRE(n_pairs > 0 && n_c > 0 && l > 0 && npp >= n_pairs && cell_stride >= 0, "hypel_svm_scatter_coef_f32");
    HYPEL_REQUIRE((int64_t)n_c * npp <= INT32_MAX && ldc >= (int64_t)n_c * npp, "hypel_svm_scatter_coef_f32: ldc < n_c * npp");
    hipLaunchKernelGGL(svm_scatter_coef_kernel, dim3(hypel_grid_1d((int64_t)l * n_c * npp, SVM_THREADS)), dim3(SVM_THREADS), 0,
                       (hipStream_t)stream, alpha_y, rho, pairs, n_pairs, n_c, cell_stride, l, npp, coef, ldc, bias);
    HYPEL_CHECK_LAUNCH("hypel_svm_scatter_coef_f32");
    return 0;
}

extern "C" int hypel_svm_vote_score(const float* dec, int64_t ld, int64_t rows, int32_t n_classes, int32_t n_cells,
                                    int32_t npp, const int32_t* truth, int32_t* correct, hypel_stream_t stream) {
    HYPEL_REQUIRE(dec && truth && correct && rows >= 0, "hypel_svm_vote_score");
    HYPEL_REQUIRE(n_classes >= 2 && n_classes <= 255,
                  "hypel_svm_vote_score: 2..255 classes (256 byte counters per class + the block's partial sums fit 64 KB of LDS)");
    HYPEL_REQUIRE(npp >= n_classes * (n_classes - 1) / 2, "hypel_svm_vote_score: npp < number of pairs");
    HYPEL_REQUIRE(n_cells > 0 && n_cells <= 65535 && ld >= (int64_t)n_cells * npp, "hypel_svm_vote_score: ld < n_cells * npp");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(svm_vote_score_kernel, dim3(hypel_grid_1d(rows, SVM_THREADS, 64), n_cells), dim3(SVM_THREADS),
                       (size_t)n_classes * SVM_THREADS, (hipStream_t)stream, dec, ld, rows, n_classes, npp, truth, correct);
    HYPEL_CHECK_LAUNCH("hypel_svm_vote_score");
    return 0;
}
