// gfx950: accuracy of the device expf / logf that softmax_xent_kernel calls, in fp32 ulps against the host's double
// exp / log, on the argument ranges tests/test_gpu_step_tail.py uses (the figures in its softmax docstring come from
// here).  Compiled like the library (no fast-math).  Standalone:
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
    return 0;
}
