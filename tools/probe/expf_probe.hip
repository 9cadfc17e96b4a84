// Measures the fast exp the flow band's convex upsample uses (__expf: exp2 of the fp32 product log2(e) x on the hardware's exp2 unit) against
// float64 exp on the softmax's argument range - the logits minus their maximum, i.e. x <= 0.  tests/raft_ref.py EXPF_REL is twice the figure
// this prints.  Build: hipcc --offload-arch=gfx950 -O3 -o expf_probe tools/probe/expf_probe.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <vector>

__global__ void probe(const float *x, float *y, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __expf(x[i]);
}

int main() {
    const int n = 1 << 22;
    std::vector<float> x(n), y(n);
    unsigned s = 12345u;
    for (int i = 0; i < n; ++i) {           // half uniform on [-20, 0] (weights that matter), half on [-170, 0] (logits of +-80 and beyond)
        s = s * 1664525u + 1013904223u;
        const double u = (double)(s >> 8) / (double)(1 << 24);
        x[i] = (float)(-(i & 1 ? 170.0 : 20.0) * u);
    }
    float *dx = nullptr, *dy = nullptr;
    if (hipMalloc(&dx, n * 4) != hipSuccess || hipMalloc(&dy, n * 4) != hipSuccess) { printf("no device memory\n"); return 1; }
    (void)hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe, dim3(n / 256), dim3(256), 0, 0, dx, dy, n);
    if (hipMemcpy(y.data(), dy, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 1; }
    double rel = 0, rel17 = 0, abs_small = 0, xr = 0;
    for (int i = 0; i < n; ++i) {
        const double t = exp((double)x[i]), e = fabs((double)y[i] - t);
        if (t >= 0x1p-126) {                 // normal results: relative error; x >= -17.33 is where a weight is >= 2^-25 of the largest
            if (e / t > rel) { rel = e / t; xr = x[i]; }
            if (x[i] >= -17.33f && e / t > rel17) rel17 = e / t;
        } else if (e > abs_small) abs_small = e;
    }
    printf("__expf vs float64 exp, %d points: max relative error %.4e = 2^%.2f (at x = %.4f); on [-17.33, 0] %.4e = 2^%.2f; "
           "max absolute error where exp(x) < 2^-126: %.3e\n", n, rel, log2(rel), xr, rel17, log2(rel17), abs_small);
    (void)hipFree(dx); (void)hipFree(dy);
    return 0;
}
