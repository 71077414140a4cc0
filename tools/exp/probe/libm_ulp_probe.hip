// gfx950: accuracy of the device expf / logf that softmax_xent_kernel calls and of the device powf that lrn_fwd_kernel /
// lrn_bwd_kernel call, in fp32 ulps against the host's double exp / log / pow, on the argument ranges
// tests/test_gpu_step_tail.py and tests/head_kernel_cases.py use (the figures in the softmax docstring and the
// POWF_ULP_MEASURED table of tests/test_gpu_head_kernels.py come from here).  Compiled like the library (no fast-math).
// Standalone:
//   hipcc --offload-arch=gfx950 -O3 -o libm_ulp_probe libm_ulp_probe.hip && ./libm_ulp_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__global__ void apply(const float* x, float* e, float* l, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        e[i] = expf(x[i]);
        l[i] = logf(x[i]);
    }
}

// the two calls of the LRN kernels: powf(s, -beta) and powf(s, -beta - 1.0f), the exponent formed in fp32 as there
__global__ void apply_pow(const float* s, float beta, float* p0, float* p1, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        p0[i] = powf(s[i], -beta);
        p1[i] = powf(s[i], -beta - 1.0f);
    }
}

static double ulp_of(double ref) {  // spacing of fp32 at |ref| (subnormal spacing below FLT_MIN)
    const float r = fabsf((float)ref);
    const float up = nextafterf(r, INFINITY);
    return (double)up - (double)r;
}

static int run(const char* what, const std::vector<float>& x, bool is_exp) {
    const int n = (int)x.size();
    float *dx, *de, *dl;
    CK(hipMalloc(&dx, n * sizeof(float)));
    CK(hipMalloc(&de, n * sizeof(float)));
    CK(hipMalloc(&dl, n * sizeof(float)));
    CK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(apply, dim3((n + 255) / 256), dim3(256), 0, 0, dx, de, dl, n);
    CK(hipGetLastError());
    std::vector<float> got(n);
    CK(hipMemcpy(got.data(), is_exp ? de : dl, n * sizeof(float), hipMemcpyDeviceToHost));
    double worst = 0.0;
    float worst_x = 0.0f;
    int nonzero = 0;
    for (int i = 0; i < n; ++i) {
        const double ref = is_exp ? exp((double)x[i]) : log((double)x[i]);
        const double err = fabs((double)got[i] - ref) / ulp_of(ref);
        if (err > worst) { worst = err; worst_x = x[i]; }
        nonzero += got[i] != 0.0f;
    }
    printf("%-28s n=%d  max error %.4f ulp (at x=%.9g)  non-zero results: %d\n", what, n, worst, worst_x, nonzero);
    CK(hipFree(dx)); CK(hipFree(de)); CK(hipFree(dl));
    return 0;
}

// n arguments spread evenly in log(s) over [lo, hi]; one line per exponent
static int run_pow(float beta, double lo, double hi, int n) {
    std::vector<float> s(n);
    for (int i = 0; i < n; ++i) s[i] = (float)(lo * exp(log(hi / lo) * (i + 0.37) / n));
    float *ds, *d0, *d1;
    CK(hipMalloc(&ds, n * sizeof(float)));
    CK(hipMalloc(&d0, n * sizeof(float)));
    CK(hipMalloc(&d1, n * sizeof(float)));
    CK(hipMemcpy(ds, s.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(apply_pow, dim3((n + 255) / 256), dim3(256), 0, 0, ds, beta, d0, d1, n);
    CK(hipGetLastError());
    std::vector<float> g0(n), g1(n);
    CK(hipMemcpy(g0.data(), d0, n * sizeof(float), hipMemcpyDeviceToHost));
    CK(hipMemcpy(g1.data(), d1, n * sizeof(float), hipMemcpyDeviceToHost));
    for (int which = 0; which < 2; ++which) {
        const float e = which ? -beta - 1.0f : -beta;
        const std::vector<float>& got = which ? g1 : g0;
        double worst = 0.0, smallest = INFINITY;
        float worst_s = 0.0f;
        for (int i = 0; i < n; ++i) {
            const double ref = pow((double)s[i], (double)e);
            const double err = fabs((double)got[i] - ref) / ulp_of(ref);
            if (err > worst) { worst = err; worst_s = s[i]; }
            if (ref < smallest) smallest = ref;
        }
        printf("powf(s, %-5g) on [%g, %g]  n=%d  max error %.4f ulp (at s=%.9g)  smallest result %.3g\n", (double)e, lo, hi,
               n, worst, worst_s, smallest);
    }
    CK(hipFree(ds)); CK(hipFree(d0)); CK(hipFree(d1));
    return 0;
}

int main() {
    const int n = 8192;
    std::vector<float> a(n), b(n), c(n), d(n);
    for (int i = 0; i < n; ++i) {
        const double t = (i + 0.37) / n;
        a[i] = (float)(-87.0 * t);                 // expf, normal results
        b[i] = (float)(-87.0 - 17.0 * t);          // expf, subnormal results down to the underflow at about -103.97
        c[i] = (float)(-104.5 - 10000.0 * t * t);  // expf, past the underflow: exactly 0
        d[i] = (float)(1.0 + 15.0 * t);            // logf on [1, 16]: a sum of c <= 15 terms, the largest of them 1
    }
    if (run("expf on [-87, 0]", a, true)) return 1;
    if (run("expf on [-104, -87]", b, true)) return 1;
    if (run("expf on [-10104.5, -104.5]", c, true)) return 1;
    if (run("logf on [1, 16]", d, false)) return 1;
    // LRN: s = bias + alpha * (window sum of x^2) >= bias.  (beta, bias) = (0.5, 1) and (0.75, 2), the two parameter
    // sets of tests/head_kernel_cases.py; s about the bias (operands of 1e-3), up to 1e11 (a 384-wide window of
    // operands of 1e3 squared: 4e8 .. 1e10), and 1e25 .. 1e31 (one operand of 1e15 per row: 1e26 at alpha = 1e-4, 1e30
    // at alpha = 1, where powf(s, -1.5) and powf(s, -1.75) end among the subnormals or underflow)
    const float betas[2] = {0.5f, 0.75f};
    const double biases[2] = {1.0, 2.0};
    for (int k = 0; k < 2; ++k) {
        if (run_pow(betas[k], biases[k], 1.01 * biases[k], n)) return 1;
        if (run_pow(betas[k], biases[k], 1e11, n)) return 1;
        if (run_pow(betas[k], 1e25, 1e31, n)) return 1;
    }
    return 0;
}
