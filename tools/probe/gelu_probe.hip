// Measures the GEMM epilogue's GELU (gemm_kernels.h fast_gelu2: a degree-5 fit of log2 Q(|x|) and one exp2) against the float64 erf form
// 0.5 x (1 + erf(x / sqrt 2)) on [-8, 8].  tests/epi_ref.py holds the absolute figure this prints as GELU_ABS_MEASURED and allows twice that.
// Build: hipcc --offload-arch=gfx950 -O3 -Iinclude -o gelu_probe tools/probe/gelu_probe.hip
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../../prisma_amd/csrc/gemm_kernels.h"

__global__ void probe(const float *x, float *y, int n) {
    const int i = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (i + 1 < n) {
        float a = x[i], b = x[i + 1];
        fast_gelu2(a, b);
        y[i] = a; y[i + 1] = b;
    }
}

int main() {
    const int n = 1 << 22;
    std::vector<float> x(n), y(n);
    for (int i = 0; i < n; ++i) x[i] = (float)(-8.0 + 16.0 * (double)i / (double)(n - 1));
    float *dx = nullptr, *dy = nullptr;
    if (hipMalloc(&dx, n * 4) != hipSuccess || hipMalloc(&dy, n * 4) != hipSuccess) { printf("no device memory\n"); return 1; }
    (void)hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe, dim3(n / 512), dim3(256), 0, 0, dx, dy, n);
    if (hipMemcpy(y.data(), dy, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 1; }
    double worst = 0, at = 0, rel = 0, rel_at = 0;
    for (int i = 0; i < n; ++i) {
        const double t = 0.5 * (double)x[i] * (1.0 + erf((double)x[i] / sqrt(2.0))), e = fabs((double)y[i] - t);
        if (e > worst) { worst = e; at = x[i]; }
        if (fabs(t) > 0x1p-20 && e / fabs(t) > rel) { rel = e / fabs(t); rel_at = x[i]; }
    }
    printf("fast_gelu2 vs float64 erf-GELU on [-8, 8], %d points: max absolute error %.4e = 2^%.2f (at x = %.4f); max relative error where "
           "|gelu| > 2^-20: %.4e (at x = %.4f)\n", n, worst, log2(worst), at, rel, rel_at);
    (void)hipFree(dx); (void)hipFree(dy);
    return 0;
}
