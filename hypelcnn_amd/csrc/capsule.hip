// Capsule classifier (CAPModel): per-capsule prediction vectors, dynamic routing, label mask.  gfx950, wave64, fp32 tensors.
//
// Shapes: batch N, primary capsules I, classes J, capsule width D, JD = J * D prediction columns.
//   x[n][i][d]      primary capsules, a VIEW of a pixel-major buffer: pix[i / M] + n * ldx + (i % M) * D + d
//   W[i][d][jd]     one [D x JD] map per capsule (the I variables are one contiguous slab), bias[i][jd]
//   u_hat[n][i][jd] prediction vectors (the only large tensor: N * I * JD floats)
//   coef[i][j]      routing coefficients c_r (or, backward, db_r);  vec[n][jd]  s_r / v_r / ds_r
//
// Everything behind the u_hat product is bound by the passes over u_hat.  Every sum over i or n is taken inside one block
// in a fixed order (per-wave strided partial sums, then the waves in wave order): no atomics, two runs give the same bits.
#include "common.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int kWave = 64;
constexpr int kRouteWaves = 8;   // caps_route_*: waves per block, each walks the capsules i = wave, wave + 8, ...
constexpr int kAgreeWaves = 4;   // caps_agree_*: waves per block, each walks the samples n = wave, wave + 4, ...
constexpr int kMaxSlots = HYPEL_CAPS_MAX_JD / kWave;  // columns a lane owns in caps_agree_*
constexpr int kTileN = 16;       // samples per staged tile of the u_hat products
constexpr float kSquashEps = 1e-9f;

// squash of one capsule: v = q * s / ((1 + q) * sqrt(q + eps)), q = mean(s^2) (CAPModel.py:99-100: a mean, not a sum)
__device__ __forceinline__ float squash_gain(float q) { return q / ((1.0f + q) * sqrtf(q + kSquashEps)); }

// d gain / d q = ((q + eps) - q (1 + q) / 2) / ((1 + q)^2 (q + eps)^1.5)
__device__ __forceinline__ float squash_gain_grad(float q) {
    const float qe = q + kSquashEps;
    return (qe - 0.5f * q * (1.0f + q)) / ((1.0f + q) * (1.0f + q) * qe * sqrtf(qe));
}

// ds = gain * dv + gain' * (2 / D) * <s, dv> * s for the D values at s / dv (stride 1); writes ds
__device__ __forceinline__ void squash_bwd(const float* s, const float* dv, int D, float* ds) {
    float q = 0.0f, dot = 0.0f;
    for (int e = 0; e < D; ++e) {
        q += s[e] * s[e];
        dot += s[e] * dv[e];
    }
    q /= (float)D;
    const float g = squash_gain(q);
    const float k = squash_gain_grad(q) * (2.0f / (float)D) * dot;
    for (int e = 0; e < D; ++e) ds[e] = g * dv[e] + k * s[e];
}

// ------------------------------------------------------------------------------------------------ u_hat forward
// One block per capsule i: W_i and bias_i go to LDS once, then the batch in tiles of kTileN samples.
// u_hat[n][i][col] = bias_i[col] + sum_d x[n][i][d] * W_i[d][col].  Dynamic LDS: (D + 1) * JD + kTileN * D floats.
__global__ __launch_bounds__(256) void caps_uhat_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ pix,
                                                             int64_t ldx, int M, const float* __restrict__ W,
                                                             const float* __restrict__ bias, int64_t N, int I, int D,
                                                             int JD, float* __restrict__ uhat) {
    extern __shared__ float lds[];
    float* Ws = lds;              // [D][JD]
    float* bs = Ws + D * JD;      // [JD]
    float* xs = bs + JD;          // [kTileN][D]
    const int i = blockIdx.x;
    const int tid = threadIdx.x;
    const float* Wi = W + (int64_t)i * D * JD;
    for (int k = tid; k < D * JD; k += 256) Ws[k] = Wi[k];
    for (int k = tid; k < JD; k += 256) bs[k] = bias[(int64_t)i * JD + k];
    const int64_t xbase = pix[i / M] + (int64_t)(i % M) * D;
    for (int64_t n0 = 0; n0 < N; n0 += kTileN) {
        const int tn = (int)((N - n0) < kTileN ? (N - n0) : kTileN);
        __syncthreads();
        for (int k = tid; k < tn * D; k += 256) xs[k] = x[xbase + (n0 + k / D) * ldx + k % D];
        __syncthreads();
        for (int col = tid; col < JD; col += 256) {
            for (int t = 0; t < tn; ++t) {
                float acc = bs[col];
                for (int d = 0; d < D; ++d) acc += xs[t * D + d] * Ws[d * JD + col];
                uhat[((n0 + t) * I + i) * (int64_t)JD + col] = acc;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ sum over the capsules
// out[n][col] = sum_i coef[i][col / D] * u_hat[n][i][col].  Block = (column group, sample n); a column group is
// CW = (64 / D) * D columns (whole capsules), one lane per column; wave w sums i = w, w + 8, ... and the waves are added
// in wave order.  Epilogue per capsule of the group (one thread each):
//   FORWARD:  s = out, v = squash(s), y[n][j] = |v|  (y may be null)
//   BACKWARD: out = dv, ds = squash'(s_in) dv
template <bool FORWARD>
__global__ __launch_bounds__(kRouteWaves * kWave) void caps_route_kernel(
    const float* __restrict__ uhat, const float* __restrict__ coef, int I, int J, int D, float* __restrict__ s_out,
    float* __restrict__ v_out, float* __restrict__ y_out, const float* __restrict__ s_in, float* __restrict__ ds_out) {
    __shared__ float part[kRouteWaves][kWave];
    __shared__ float tot[kWave];
    const int JD = J * D;
    const int cw = (kWave / D) * D;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int64_t n = blockIdx.y;
    const int col = blockIdx.x * cw + lane;
    const bool live = lane < cw && col < JD;
    float acc = 0.0f;
    if (live) {
        const int j = col / D;
        const float* u = uhat + n * (int64_t)I * JD + col;
        int i = wave;
        for (; i + 3 * kRouteWaves < I; i += 4 * kRouteWaves) {  // four loads in flight per lane
            const float u0 = u[(int64_t)i * JD], u1 = u[(int64_t)(i + kRouteWaves) * JD];
            const float u2 = u[(int64_t)(i + 2 * kRouteWaves) * JD], u3 = u[(int64_t)(i + 3 * kRouteWaves) * JD];
            acc += coef[(int64_t)i * J + j] * u0;
            acc += coef[(int64_t)(i + kRouteWaves) * J + j] * u1;
            acc += coef[(int64_t)(i + 2 * kRouteWaves) * J + j] * u2;
            acc += coef[(int64_t)(i + 3 * kRouteWaves) * J + j] * u3;
        }
        for (; i < I; i += kRouteWaves) acc += coef[(int64_t)i * J + j] * u[(int64_t)i * JD];
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
        float t = 0.0f;
        for (int w = 0; w < kRouteWaves; ++w) t += part[w][lane];
        tot[lane] = t;
    }
    __syncthreads();
    // one thread per capsule of the group
    const int caps = cw / D;
    if ((int)threadIdx.x < caps) {
        const int c0 = threadIdx.x * D;           // first column of this capsule inside the group
        const int gcol = blockIdx.x * cw + c0;    // ... and inside the row
        if (gcol < JD) {
            const int64_t o = n * JD + gcol;
            if (FORWARD) {
                float q = 0.0f;
                for (int e = 0; e < D; ++e) q += tot[c0 + e] * tot[c0 + e];
                q /= (float)D;
                const float g = squash_gain(q);
                float nv = 0.0f;
                for (int e = 0; e < D; ++e) {
                    const float v = g * tot[c0 + e];
                    s_out[o + e] = tot[c0 + e];
                    v_out[o + e] = v;
                    nv += v * v;
                }
                if (y_out) y_out[n * J + gcol / D] = sqrtf(nv);
            } else {
                float sv[HYPEL_CAPS_MAX_D], dsv[HYPEL_CAPS_MAX_D];
                for (int e = 0; e < D; ++e) sv[e] = s_in[o + e];
                squash_bwd(sv, tot + c0, D, dsv);
                for (int e = 0; e < D; ++e) ds_out[o + e] = dsv[e];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ sum over the batch
// a[i][j] = sum_n sum_e u_hat[n][i][j*D + e] * vec[n][j*D + e].  One block per capsule i; a lane owns the columns
// lane, lane + 64, ...; wave w sums n = w, w + 4, ...; then the waves in wave order, then the D columns of a class.
// The sums, the routing logits b and the softmax run in fp64 (like the statistics finalisers of the library): b grows
// with the batch (hundreds at batch 128), where an fp32 ulp of b is already 1e-5 of every coefficient, and the softmax
// backward of a saturated row is a difference of nearly equal numbers.  The kernels stay bound by their one read of u_hat.
//   FORWARD:  b_out = b_in + a (b_in null = 0; fp64 buffers), c_out = softmax_j(b_out)
//   BACKWARD: a = dc; db_out[j] = c[j] * sum_k c[k] (dc[j] - dc[k]) + db_next[j] (db_next null = 0) -- the softmax
//             backward c[j] (dc[j] - <c, dc>) with sum_k c[k] = 1 used to take the difference before the products
template <bool FORWARD>
__global__ __launch_bounds__(kAgreeWaves * kWave) void caps_agree_kernel(
    const float* __restrict__ uhat, const float* __restrict__ vec, int64_t N, int I, int J, int D,
    const double* __restrict__ b_in, double* __restrict__ b_out, const float* __restrict__ c_in,
    const float* __restrict__ db_next, float* __restrict__ out) {
    __shared__ double part[kAgreeWaves][HYPEL_CAPS_MAX_JD];
    __shared__ double a[HYPEL_CAPS_MAX_JD];  // per class (J <= JD)
    const int JD = J * D;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int i = blockIdx.x;
    double acc[kMaxSlots];
#pragma unroll
    for (int k = 0; k < kMaxSlots; ++k) acc[k] = 0.0;
    for (int64_t n = wave; n < N; n += kAgreeWaves) {
        const float* u = uhat + (n * I + i) * (int64_t)JD;
        const float* v = vec + n * JD;
#pragma unroll
        for (int k = 0; k < kMaxSlots; ++k) {
            const int col = k * kWave + lane;
            if (col < JD) acc[k] += (double)u[col] * (double)v[col];
        }
    }
#pragma unroll
    for (int k = 0; k < kMaxSlots; ++k) {
        const int col = k * kWave + lane;
        if (col < JD) part[wave][col] = acc[k];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < J; j += kAgreeWaves * kWave) {
        double t = 0.0;
        for (int e = 0; e < D; ++e) {
            double c = 0.0;
            for (int w = 0; w < kAgreeWaves; ++w) c += part[w][j * D + e];
            t += c;
        }
        a[j] = t;
    }
    __syncthreads();
    const int64_t o = (int64_t)i * J;
    if (FORWARD) {
        if (threadIdx.x == 0) {  // J is a handful of classes: one thread, fixed order
            double mx = -INFINITY;
            for (int j = 0; j < J; ++j) {
                const double b = (b_in ? b_in[o + j] : 0.0) + a[j];
                b_out[o + j] = b;
                a[j] = b;
                mx = fmax(mx, b);
            }
            double z = 0.0;
            for (int j = 0; j < J; ++j) {
                a[j] = exp(a[j] - mx);
                z += a[j];
            }
            for (int j = 0; j < J; ++j) out[o + j] = (float)(a[j] / z);
        }
    } else {
        for (int j = threadIdx.x; j < J; j += kAgreeWaves * kWave) {
            double t = 0.0;
            for (int k = 0; k < J; ++k) t += (double)c_in[o + k] * (a[j] - a[k]);
            out[o + j] = (float)((double)c_in[o + j] * t + (db_next ? (double)db_next[o + j] : 0.0));
        }
    }
}

// ------------------------------------------------------------------------------------------------ head of the backward
// dv[n][j][:] = gy[n][j] * v / |v| + gv[n][j][:], v = squash(s);  ds = squash'(s) dv.  One thread per (n, j).
__global__ __launch_bounds__(256) void caps_head_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ gv,
                                                             const float* __restrict__ s, int64_t N, int J, int D,
                                                             float* __restrict__ ds) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * J) return;
    const int64_t o = idx * D;
    float sv[HYPEL_CAPS_MAX_D], dv[HYPEL_CAPS_MAX_D], dsv[HYPEL_CAPS_MAX_D];
    float q = 0.0f;
    for (int e = 0; e < D; ++e) {
        sv[e] = s[o + e];
        q += sv[e] * sv[e];
    }
    const float g = squash_gain(q / (float)D);
    float nv = 0.0f;
    for (int e = 0; e < D; ++e) nv += (g * sv[e]) * (g * sv[e]);
    nv = sqrtf(nv);
    const float k = (gy && nv > 0.0f) ? gy[idx] / nv : 0.0f;
    for (int e = 0; e < D; ++e) dv[e] = k * g * sv[e] + (gv ? gv[o + e] : 0.0f);
    squash_bwd(sv, dv, D, dsv);
    for (int e = 0; e < D; ++e) ds[o + e] = dsv[e];
}

// ------------------------------------------------------------------------------------------------ u_hat backward
// du_hat[n][i][col] = sum_t coefs[t][i][col / D] * vecs[t][n][col] is built on the fly (never stored).  One block per
// capsule i, the batch in tiles of kTileN samples:
//   dbias_i[col] = sum_n du,  dW_i[d][col] = sum_n x[n][i][d] * du      (thread = column, registers)
//   dx[n][i][d]  = sum_col du[n][col] * W_i[d][col]                        (thread = (sample of the tile, d), from LDS)
// Dynamic LDS: D * JDP + kTileN * JDP + kTileN * D + T * J floats, JDP = JD | 1 (odd row stride: no bank conflicts).
__global__ __launch_bounds__(256) void caps_uhat_bwd_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ pix, int64_t ldx, int M, const float* __restrict__ W,
    int64_t N, int I, int J, int D, int T, const float* __restrict__ coefs, const float* __restrict__ vecs,
    float* __restrict__ dW, float* __restrict__ dbias, int acc_w, float* __restrict__ dx,
    const int64_t* __restrict__ dpix, int64_t lddx, int acc_x) {
    extern __shared__ float lds[];
    const int JD = J * D;
    const int JDP = JD | 1;
    float* Ws = lds;                    // [D][JDP]
    float* dus = Ws + D * JDP;          // [kTileN][JDP]
    float* xs = dus + kTileN * JDP;     // [kTileN][D]
    float* cs = xs + kTileN * D;        // [T][J]
    const int i = blockIdx.x;
    const int tid = threadIdx.x;
    const float* Wi = W + (int64_t)i * D * JD;
    for (int k = tid; k < D * JD; k += 256) Ws[(k / JD) * JDP + k % JD] = Wi[k];
    for (int k = tid; k < T * J; k += 256) cs[k] = coefs[((int64_t)(k / J) * I + i) * J + k % J];
    const int64_t xbase = pix[i / M] + (int64_t)(i % M) * D;
    const int64_t dxbase = dx ? dpix[i / M] + (int64_t)(i % M) * D : 0;
    // a thread owns the columns tid and tid + 256 (JD <= 512)
    float gw[2][HYPEL_CAPS_MAX_D], gb[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        gb[k] = 0.0f;
#pragma unroll
        for (int d = 0; d < HYPEL_CAPS_MAX_D; ++d) gw[k][d] = 0.0f;
    }
    for (int64_t n0 = 0; n0 < N; n0 += kTileN) {
        const int tn = (int)((N - n0) < kTileN ? (N - n0) : kTileN);
        __syncthreads();
        for (int k = tid; k < tn * D; k += 256) xs[k] = x[xbase + (n0 + k / D) * ldx + k % D];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int col = k * 256 + tid;
            if (col < JD) {
                const int j = col / D;
                for (int t = 0; t < tn; ++t) {
                    float du = 0.0f;
                    for (int q = 0; q < T; ++q) du += cs[q * J + j] * vecs[((int64_t)q * N + n0 + t) * JD + col];
                    dus[t * JDP + col] = du;
                    gb[k] += du;
#pragma unroll
                    for (int d = 0; d < HYPEL_CAPS_MAX_D; ++d)
                        if (d < D) gw[k][d] += xs[t * D + d] * du;
                }
            }
        }
        __syncthreads();
        if (dx) {
            for (int k = tid; k < tn * D; k += 256) {
                const int t = k / D, d = k % D;
                float acc = 0.0f;
                for (int col = 0; col < JD; ++col) acc += dus[t * JDP + col] * Ws[d * JDP + col];
                float* p = dx + dxbase + (n0 + t) * lddx + d;
                *p = acc_x ? *p + acc : acc;
            }
        }
    }
    if (dW) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int col = k * 256 + tid;
            if (col < JD) {
                float* pb = dbias + (int64_t)i * JD + col;
                *pb = acc_w ? *pb + gb[k] : gb[k];
#pragma unroll
                for (int d = 0; d < HYPEL_CAPS_MAX_D; ++d)
                    if (d < D) {
                        float* pw = dW + ((int64_t)i * D + d) * JD + col;
                        *pw = acc_w ? *pw + gw[k][d] : gw[k][d];
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ label mask
__global__ __launch_bounds__(256) void caps_mask_fwd_kernel(const float* __restrict__ v, int64_t ldv,
                                                             const float* __restrict__ labels, int64_t ldl, int64_t N,
                                                             int J, int D, float* __restrict__ out, int64_t ldo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * D) return;
    const int64_t n = idx / D;
    const int e = (int)(idx % D);
    float acc = 0.0f;
    for (int j = 0; j < J; ++j) acc += labels[n * ldl + j] * v[n * ldv + j * D + e];
    out[n * ldo + e] = acc;
}

__global__ __launch_bounds__(256) void caps_mask_bwd_kernel(const float* __restrict__ gout, int64_t ldg,
                                                             const float* __restrict__ labels, int64_t ldl, int64_t N,
                                                             int J, int D, float* __restrict__ gv, int64_t ldgv, int acc) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int JD = J * D;
    if (idx >= N * JD) return;
    const int64_t n = idx / JD;
    const int col = (int)(idx % JD);
    const float g = labels[n * ldl + col / D] * gout[n * ldg + col % D];
    float* p = gv + n * ldgv + col;
    *p = acc ? *p + g : g;
}

bool caps_shape_ok(int64_t N, int I, int J, int D) {
    return N > 0 && N <= HYPEL_CAPS_MAX_N && I > 0 && J > 0 && D > 0 && D <= HYPEL_CAPS_MAX_D && (int64_t)J * D <= HYPEL_CAPS_MAX_JD;
}

constexpr size_t kMaxDynLds = HYPEL_CAPS_MAX_LDS;  // graph.py::capsule_fits restates the two LDS formulas below

}  // namespace

extern "C" int hypel_caps_uhat_fwd(const float* x, const int64_t* pix, int64_t ldx, int32_t m, const float* w,
                                   const float* bias, int64_t n, int32_t i, int32_t d, int32_t jd, float* uhat,
                                   hypel_stream_t stream) {
    HYPEL_REQUIRE(x && pix && w && bias && uhat && m > 0 && d > 0 && jd > 0 && jd % d == 0 && i % m == 0 &&
                      caps_shape_ok(n, i, jd / d, d),
                  "hypel_caps_uhat_fwd");
    const size_t lds = sizeof(float) * ((size_t)(d + 1) * jd + (size_t)kTileN * d);
    HYPEL_REQUIRE(lds <= kMaxDynLds, "hypel_caps_uhat_fwd");
    hipLaunchKernelGGL(caps_uhat_fwd_kernel, dim3(i), dim3(256), lds, ST, x, pix, ldx, m, w, bias, n, i, d, jd, uhat);
    HYPEL_CHECK_LAUNCH("hypel_caps_uhat_fwd");
    return 0;
}

extern "C" int hypel_caps_route_fwd(const float* uhat, const float* coef, int64_t n, int32_t i, int32_t j, int32_t d,
                                    float* s, float* v, float* y, hypel_stream_t stream) {
    HYPEL_REQUIRE(uhat && coef && s && v && caps_shape_ok(n, i, j, d), "hypel_caps_route_fwd");
    const int cw = (kWave / d) * d;
    hipLaunchKernelGGL(caps_route_kernel<true>, dim3((j * d + cw - 1) / cw, (unsigned)n), dim3(kRouteWaves * kWave), 0, ST,
                       uhat, coef, i, j, d, s, v, y, (const float*)nullptr, (float*)nullptr);
    HYPEL_CHECK_LAUNCH("hypel_caps_route_fwd");
    return 0;
}

extern "C" int hypel_caps_route_bwd(const float* uhat, const float* coef, int64_t n, int32_t i, int32_t j, int32_t d,
                                    const float* s_in, float* ds_out, hypel_stream_t stream) {
    HYPEL_REQUIRE(uhat && coef && s_in && ds_out && caps_shape_ok(n, i, j, d), "hypel_caps_route_bwd");
    const int cw = (kWave / d) * d;
    hipLaunchKernelGGL(caps_route_kernel<false>, dim3((j * d + cw - 1) / cw, (unsigned)n), dim3(kRouteWaves * kWave), 0,
                       ST, uhat, coef, i, j, d, (float*)nullptr, (float*)nullptr, (float*)nullptr, s_in, ds_out);
    HYPEL_CHECK_LAUNCH("hypel_caps_route_bwd");
    return 0;
}

extern "C" int hypel_caps_agree_fwd(const float* uhat, const float* v, int64_t n, int32_t i, int32_t j, int32_t d,
                                    const double* b_in, double* b_out, float* c_out, hypel_stream_t stream) {
    HYPEL_REQUIRE(uhat && v && b_out && c_out && caps_shape_ok(n, i, j, d), "hypel_caps_agree_fwd");
    hipLaunchKernelGGL(caps_agree_kernel<true>, dim3(i), dim3(kAgreeWaves * kWave), 0, ST, uhat, v, n, i, j, d, b_in,
                       b_out, (const float*)nullptr, (const float*)nullptr, c_out);
    HYPEL_CHECK_LAUNCH("hypel_caps_agree_fwd");
    return 0;
}

extern "C" int hypel_caps_agree_bwd(const float* uhat, const float* ds, int64_t n, int32_t i, int32_t j, int32_t d,
                                    const float* c, const float* db_next, float* db, hypel_stream_t stream) {
    HYPEL_REQUIRE(uhat && ds && c && db && caps_shape_ok(n, i, j, d), "hypel_caps_agree_bwd");
    hipLaunchKernelGGL(caps_agree_kernel<false>, dim3(i), dim3(kAgreeWaves * kWave), 0, ST, uhat, ds, n, i, j, d,
                       (const double*)nullptr, (double*)nullptr, c, db_next, db);
    HYPEL_CHECK_LAUNCH("hypel_caps_agree_bwd");
    return 0;
}

extern "C" int hypel_caps_head_bwd(const float* gy, const float* gv, const float* s, int64_t n, int32_t j, int32_t d,
                                   float* ds, hypel_stream_t stream) {
    HYPEL_REQUIRE((gy || gv) && s && ds && caps_shape_ok(n, 1, j, d), "hypel_caps_head_bwd");
    hipLaunchKernelGGL(caps_head_bwd_kernel, dim3((unsigned)((n * j + 255) / 256)), dim3(256), 0, ST, gy, gv, s, n, j, d,
                       ds);
    HYPEL_CHECK_LAUNCH("hypel_caps_head_bwd");
    return 0;
}

extern "C" int hypel_caps_uhat_bwd(const float* x, const int64_t* pix, int64_t ldx, int32_t m, const float* w, int64_t n,
                                   int32_t i, int32_t j, int32_t d, int32_t n_terms, const float* coefs,
                                   const float* vecs, float* dw, float* dbias, int32_t acc_w, float* dx,
                                   const int64_t* dpix, int64_t lddx, int32_t acc_x, hypel_stream_t stream) {
    HYPEL_REQUIRE(x && pix && w && coefs && vecs && m > 0 && n_terms > 0 && i % m == 0 && caps_shape_ok(n, i, j, d) &&
                      (dw == nullptr) == (dbias == nullptr) && (dx == nullptr || dpix != nullptr) && (dw || dx),
                  "hypel_caps_uhat_bwd");
    const int jdp = (j * d) | 1;
    const size_t lds = sizeof(float) * ((size_t)d * jdp + (size_t)kTileN * jdp + (size_t)kTileN * d + (size_t)n_terms * j);
    HYPEL_REQUIRE(lds <= kMaxDynLds, "hypel_caps_uhat_bwd");
    hipLaunchKernelGGL(caps_uhat_bwd_kernel, dim3(i), dim3(256), lds, ST, x, pix, ldx, m, w, n, i, j, d, n_terms, coefs,
                       vecs, dw, dbias, acc_w, dx, dpix, lddx, acc_x);
    HYPEL_CHECK_LAUNCH("hypel_caps_uhat_bwd");
    return 0;
}

extern "C" int hypel_caps_mask_fwd(const float* v, int64_t ldv, const float* labels, int64_t ldl, int64_t n, int32_t j,
                                   int32_t d, float* out, int64_t ldo, hypel_stream_t stream) {
    HYPEL_REQUIRE(v && labels && out && n > 0 && j > 0 && d > 0, "hypel_caps_mask_fwd");
    hipLaunchKernelGGL(caps_mask_fwd_kernel, dim3((unsigned)((n * d + 255) / 256)), dim3(256), 0, ST, v, ldv, labels, ldl,
                       n, j, d, out, ldo);
    HYPEL_CHECK_LAUNCH("hypel_caps_mask_fwd");
    return 0;
}

extern "C" int hypel_caps_mask_bwd(const float* gout, int64_t ldg, const float* labels, int64_t ldl, int64_t n, int32_t j,
                                   int32_t d, float* gv, int64_t ldgv, int32_t accumulate, hypel_stream_t stream) {
    HYPEL_REQUIRE(gout && labels && gv && n > 0 && j > 0 && d > 0, "hypel_caps_mask_bwd");
    hipLaunchKernelGGL(caps_mask_bwd_kernel, dim3((unsigned)((n * (int64_t)j * d + 255) / 256)), dim3(256), 0, ST, gout,
                       ldg, labels, ldl, n, j, d, gv, ldgv, accumulate);
    HYPEL_CHECK_LAUNCH("hypel_caps_mask_bwd");
    return 0;
}
