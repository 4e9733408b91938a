// rp_math_sc_test.hip -- the scalar-coefficient paths of rp_math.h (rp_atan<true>, rp_sincos<true>: what the four-wave instance of
// rp_eval_kernel's fixed-stride variant runs) next to the plain ones, for tests/test_gpu_math_scalar_coeffs.py
// (TEST HELPER, not part of the product ABI; built as lib/librp_mathsctest.so).
#include <hip/hip_runtime.h>
#include "rp_math.h"

// out[0 .. n) the plain function, out[n .. 2n) the scalar-coefficient one; kind 0: atan, 1: sin, cos (out2 likewise).
// Lanes behind n evaluate lane-0-of-the-wavefront's input, so that the padding does not decide a wave-uniform branch.
template <bool SC>
__device__ __forceinline__ void math_one(int kind, double x, double &a, double &b) {
    if (kind == 0) a = rp_atan<SC>(x);
    else rp_sincos<SC>(x, &a, &b);
}

__global__ __launch_bounds__(64) void k_math_sc(int kind, int n, const double *in, double *out, double *out2) {
    const int i = blockIdx.x * 64 + threadIdx.x;   // one wavefront per workgroup: wavefront w holds in[64 w .. 64 w + 63]
    const double x = in[i < n ? i : blockIdx.x * 64];
    double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;
    math_one<false>(kind, x, a0, b0);
    math_one<true>(kind, x, a1, b1);
    if (i < n) {
        out[i] = a0; out[n + i] = a1;
        out2[i] = b0; out2[n + i] = b1;
    }
}

extern "C" int rpt_math_sc(int kind, int n, const double *in, double *out, double *out2) {
    if (n <= 0 || (kind != 0 && kind != 1)) return -3;
    double *d_in = nullptr, *d_out = nullptr, *d_out2 = nullptr;
    if (hipMalloc((void **)&d_in, sizeof(double) * n) != hipSuccess) return -1;
    if (hipMalloc((void **)&d_out, sizeof(double) * 2 * n) != hipSuccess) return -1;
    if (hipMalloc((void **)&d_out2, sizeof(double) * 2 * n) != hipSuccess) return -1;
    hipError_t e = hipMemcpy(d_in, in, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_out2, 0, sizeof(double) * 2 * n);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_math_sc, dim3((n + 63) / 64), dim3(64), 0, 0, kind, n, d_in, d_out, d_out2);
        e = hipMemcpy(out, d_out, sizeof(double) * 2 * n, hipMemcpyDeviceToHost);
    }
    if (e == hipSuccess) e = hipMemcpy(out2, d_out2, sizeof(double) * 2 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_out2);
    return e == hipSuccess ? 0 : -2;
}
