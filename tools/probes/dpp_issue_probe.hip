// hipcc --offload-arch=gfx950 -O3 -o tools/probes/dpp_issue_probe tools/probes/dpp_issue_probe.hip
// issue cost of DPP-modified VALU instructions on gfx950: N dependent-free v_fmac_f32 per wave against the same with a
// row_newbcast operand, at 1 and 6 waves per SIMD
#include <hip/hip_runtime.h>
#include <stdio.h>
#define R8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
template <int MODE>
__global__ void __launch_bounds__(256) k(float *out, int iters) {
    float a[8], s = (float)threadIdx.x * 1e-3f, w = 1.0001f;
    for (int i = 0; i < 8; ++i) a[i] = (float)i;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (MODE == 0) {
#define P(i) asm volatile("v_fmac_f32_e32 %0, %1, %2" : "+v"(a[i]) : "v"(s), "v"(w));
                R8(P)
#undef P
            } else if (MODE == 1) {
#define P(i) asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(a[i]) : "v"(s), "v"(w));
                R8(P)
#undef P
            } else if (MODE == 2) {
#define P(i) asm volatile("v_mov_b32_dpp %0, %1 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(a[i]) : "v"(s));
                R8(P)
#undef P
            } else {
#define P(i) asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(a[i]) : "v"(s), "v"(w));
                R8(P)
#undef P
            }
        }
    }
    float t = 0.f;
    for (int i = 0; i < 8; ++i) t += a[i];
    out[blockIdx.x * 256 + threadIdx.x] = t;
}
template <int MODE>
static void run(const char *name, float *out, int wps) {
    const int iters = 20000, blocks = 256 * wps;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(256), 0, 0, out, 100);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(256), 0, 0, out, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms = 0.f; hipEventElapsedTime(&ms, e0, e1);
    const double inst_per_simd = (double)iters * 64.0 * wps;
    printf("{\"probe\": \"%s\", \"waves_per_simd\": %d, \"ms\": %.4f, \"ns_per_instr_per_simd\": %.4f}\n", name, wps, ms, ms * 1e6 / inst_per_simd);
}
int main() {
    float *out; hipMalloc(&out, 256 * 8 * 256 * sizeof(float));
    for (int wps : {1, 6}) {
        run<0>("v_fmac_f32", out, wps);
        run<1>("v_fmac_f32_dpp row_newbcast", out, wps);
        run<2>("v_mov_b32_dpp row_newbcast", out, wps);
        run<3>("v_fmac_f32_dpp quad_perm", out, wps);
    }
    hipError_t e = hipDeviceSynchronize();
    printf("{\"status\": \"%s\"}\n", hipGetErrorString(e));
    return e != hipSuccess;
}
