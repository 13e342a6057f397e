// Measures the device library's erff and the fast __expf, as the kernels of csrc/ compile them, against the host's fp64 erf /
// exp: the worst error in units of the last place of the fp32 result over the sweeps the MLP-head tests use
// (tests/test_mlp_head_gpu.py: the bound of the GELU kernels allows twice these figures; DESIGN.md section 9m records them).
//   erff(t):    t on a uniform grid of 2^22 points over [-4.5, 4.5] (x = t * sqrt 2 up to +-6.36) and +-2^-k, k = 0 .. 40
//   __expf(a):  a on a uniform grid of 2^22 points over [-20.25, 0]   (a = -x^2 / 2 for |x| <= 6.36)
// Build and run (prints one JSON line):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast scripts/device_math_ulp.hip -o device_math_ulp && ./device_math_ulp
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void eval_k(const float* __restrict__ in, float* __restrict__ out, int n, int which) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = which == 0 ? erff(in[i]) : __expf(in[i]);
}

static double ulp_of(double ref) {
    if (ref == 0.0) return std::ldexp(1.0, -149);
    int e;
    std::frexp(std::fabs(ref), &e);                 // |ref| = m * 2^e, m in [0.5, 1)
    return std::ldexp(1.0, (e - 1 < -126 ? -126 : e - 1) - 23);
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("{\"error\": \"%s\"}\n", hipGetErrorString(e_)); return 1; } } while (0)

static int measure(const std::vector<float>& in, int which, double* worst, float* at) {
    const int n = (int)in.size();
    float *din = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&din, n * sizeof(float)));
    CHECK(hipMalloc(&dout, n * sizeof(float)));
    CHECK(hipMemcpy(din, in.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_k, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n, which);
    CHECK(hipGetLastError());
    std::vector<float> out(n);
    CHECK(hipMemcpy(out.data(), dout, n * sizeof(float), hipMemcpyDeviceToHost));
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    *worst = 0.0;
    *at = 0.f;
    for (int i = 0; i < n; ++i) {
        const double ref = which == 0 ? std::erf((double)in[i]) : std::exp((double)in[i]);
        const double err = std::fabs((double)out[i] - ref) / ulp_of(ref);
        if (err > *worst) { *worst = err; *at = in[i]; }
    }
    return 0;
}

int main() {
    const int N = 1 << 22;
    std::vector<float> t, a;
    for (int i = 0; i < N; ++i) t.push_back((float)(-4.5 + 9.0 * i / (N - 1)));
    for (int k = 0; k <= 40; ++k) { t.push_back(std::ldexp(1.f, -k)); t.push_back(-std::ldexp(1.f, -k)); }
    for (int i = 0; i < N; ++i) a.push_back((float)(-20.25 * i / (N - 1)));
    double we, wx;
    float ae, ax;
    if (measure(t, 0, &we, &ae) || measure(a, 1, &wx, &ax)) return 1;
    std::printf("{\"erff_worst_ulp\": %.3f, \"erff_at\": %.9g, \"fast_expf_worst_ulp\": %.3f, \"fast_expf_at\": %.9g, \"points\": %d}\n",
                we, ae, wx, ax, N);
    return 0;
}
