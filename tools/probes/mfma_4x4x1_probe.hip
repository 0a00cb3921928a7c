// hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form -o tools/probes/mfma_4x4x1_probe tools/probes/mfma_4x4x1_probe.hip
// v_mfma_f32_4x4x1_16b_f32 with cbsz:2 abid:t as the narrow forward's exponent polynomial:
//   (a) layout: which lane's A every block uses, which lane supplies B[0][j], which lane / register receives D[i][j];
//   (b) chain: six such MFMAs (1,q0) (x,qx) (y,qy) (xx,qxx) (xy,qxy) (yy,qyy) from C = 0 against power_poly() of blend_power.h,
//       bit for bit, on operands drawn the way the kernel's are and on edge sets;
//   (c) issue cost: the MFMA alone, dependent chains of six, two / four chains interleaved, chains beside independent v_fmac_f32,
//       at one and at six waves per SIMD.
// Prints one JSON object.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../splatter_a_video_amd/csrc/blend_power.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA(a, b, c, t) __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 2, t, 0)

// ---------------------------------------------------------------- (a) layout
// D = A * B with lane-identifying values: run 0 has B = 1 (D shows the lane A came from), run 1 has A = 1 (the lane of B)
__global__ void layout_kernel(float *out) {
    const int lane = threadIdx.x;
    const float id = (float)(lane + 1);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 d[2][4];
    d[0][0] = MFMA(id, 1.f, z, 0); d[0][1] = MFMA(id, 1.f, z, 1); d[0][2] = MFMA(id, 1.f, z, 2); d[0][3] = MFMA(id, 1.f, z, 3);
    d[1][0] = MFMA(1.f, id, z, 0); d[1][1] = MFMA(1.f, id, z, 1); d[1][2] = MFMA(1.f, id, z, 2); d[1][3] = MFMA(1.f, id, z, 3);
    for (int r = 0; r < 2; ++r)
        for (int t = 0; t < 4; ++t)
            for (int i = 0; i < 4; ++i) out[((r * 4 + t) * 4 + i) * 64 + lane] = d[r][t][i];
}

// ---------------------------------------------------------------- (b) chain
__device__ __forceinline__ unsigned hash32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
struct Rng {
    unsigned s;
    __device__ unsigned next() { s = hash32(s + 0x9e3779b9u); return s; }
    __device__ float uni() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }   // [0, 1)
};
enum { M_RANDOM = 0, M_INERT, M_NAN, M_DENORM, M_LARGE, M_ZERO_Q0, M_COUNT };
// counters per mode: evaluations, bit-equal, zero of the other sign (the known fma(1, -0, +0) case), both NaN with other bits,
// anything else
enum { K_TOTAL = 0, K_EQUAL, K_ZERO_SIGN, K_NAN_BITS, K_OTHER, K_COUNT };

__global__ void __launch_bounds__(64) chain_kernel(unsigned long long *cnt, float *first_bad, int mode, unsigned seed) {
    const int lane = threadIdx.x;
    Rng r{hash32(seed ^ (blockIdx.x * 64u + lane) * 2654435761u)};
    // the lane's own survivor: a random rotated conic (EWA: covariance + 0.3 I), opacity, centre within 24 pixels of the tile centre
    const float ang = 6.2831853f * r.uni();
    const float s1 = exp2f(-1.5f + 6.5f * r.uni()), s2 = exp2f(-1.5f + 6.5f * r.uni());   // standard deviations 0.35 .. 32 pixels
    const float cs = cosf(ang), sn = sinf(ang);
    float va = cs * cs * s1 * s1 + sn * sn * s2 * s2 + 0.3f, vc = sn * sn * s1 * s1 + cs * cs * s2 * s2 + 0.3f, vb = cs * sn * (s1 * s1 - s2 * s2);
    if (mode == M_LARGE) { const float k = exp2f(-14.f - 14.f * r.uni()); va *= k; vb *= k; vc *= k; }   // needle-thin: coefficients 1e4 .. 1e8
    const float det = va * vc - vb * vb;
    const float cA = vc / det, cB = -vb / det, cC = va / det;
    float o = r.uni() < 0.1f ? 1.0f : r.uni();
    const float tcx = 16.f * (float)(r.next() % 60u) + 7.5f, tcy = 16.f * (float)(r.next() % 34u) + 7.5f;   // tile centre
    float u = tcx + 48.f * r.uni() - 24.f, v = tcy + 48.f * r.uni() - 24.f;
    if (r.uni() < 0.1f) { u = tcx + floorf(16.f * r.uni()) - 7.5f; v = tcy + floorf(16.f * r.uni()) - 7.5f; }   // on a pixel centre
    if (mode == M_INERT && (r.next() & 1u)) o = 0.f;
    const PowerCoef k = power_coeffs(u, v, cA, cB, cC, o, tcx, tcy);
    float4 c0 = make_float4(k.q0, k.qx, k.qy, k.qxx), c1 = make_float4(k.qxy, k.qyy, 0.f, 0.f);
    float *cf[6] = {&c0.x, &c0.y, &c0.z, &c0.w, &c1.x, &c1.y};
    if (mode == M_NAN) {   // a NaN or an infinity in one or two of the six
        for (int n = 1 + (int)(r.next() & 1u); n > 0; --n) {
            const unsigned pick = r.next();
            *cf[pick % 6u] = (pick & 64u) ? __builtin_nanf("") : ((pick & 128u) ? __builtin_inff() : -__builtin_inff());
        }
    }
    if (mode == M_DENORM) {   // every coefficient a denormal or within a few binades of them
        for (int i = 0; i < 6; ++i) {
            const unsigned b = r.next();
            *cf[i] = __uint_as_float((b & 0x80000000u) | ((b >> 8) & 0x007fffffu) | (((b >> 4) & 3u) == 0u ? (1u << 23) * ((b >> 6) & 3u) : 0u));
        }
    }
    if (mode == M_ZERO_Q0) {
        c0.x = (r.next() & 1u) ? 0.f : -0.f;
        for (int i = 1; i < 6; ++i) {   // and some of the others +-0 as well: a zero polynomial is where the sign can show
            const unsigned b = r.next();
            if ((b & 3u) != 0u) *cf[i] = (b & 4u) ? 0.f : -0.f;
        }
    }
    // the lane's own pixel: half-integers in -7.5 .. 7.5
    const float x = (float)(r.next() & 15u) - 7.5f, y = (float)(r.next() & 15u) - 7.5f;
    const float xx = x * x, xy = x * y, yy = y * y;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 D[4];
#define CHAIN(t)                         \
    D[t] = MFMA(c0.x, 1.0f, z, t);       \
    D[t] = MFMA(c0.y, x, D[t], t);       \
    D[t] = MFMA(c0.z, y, D[t], t);       \
    D[t] = MFMA(c0.w, xx, D[t], t);      \
    D[t] = MFMA(c1.x, xy, D[t], t);      \
    D[t] = MFMA(c1.y, yy, D[t], t);
    CHAIN(0) CHAIN(1) CHAIN(2) CHAIN(3)
#undef CHAIN
    unsigned long long loc[K_COUNT] = {0, 0, 0, 0, 0};
    for (int s = 0; s < 16; ++s) {   // survivor s of the lane's 16-lane row = the lane that the forward's row_newbcast:s names
        const int src = (lane & 48) | s;
        float4 g0, g1 = make_float4(0.f, 0.f, 0.f, 0.f);
        g0.x = __shfl(c0.x, src); g0.y = __shfl(c0.y, src); g0.z = __shfl(c0.z, src); g0.w = __shfl(c0.w, src);
        g1.x = __shfl(c1.x, src); g1.y = __shfl(c1.y, src);
        const float ref = power_poly(g0, g1, x, y, xx, xy, yy);
        const float got = D[s >> 2][s & 3];
        const unsigned rb = __float_as_uint(ref), gb = __float_as_uint(got);
        int kind = K_OTHER;
        if (rb == gb) kind = K_EQUAL;
        else if (((rb | gb) & 0x7fffffffu) == 0u) kind = K_ZERO_SIGN;
        else if (ref != ref && got != got) kind = K_NAN_BITS;
        loc[K_TOTAL]++; loc[kind]++;
        if (kind == K_OTHER && atomicAdd(&cnt[M_COUNT * K_COUNT], 1ull) == 0ull) {
            const float rec[12] = {(float)mode, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, x, y, ref, got, (float)s};
            for (int i = 0; i < 12; ++i) first_bad[i] = rec[i];
        }
    }
    for (int i = 0; i < K_COUNT; ++i)
        if (loc[i]) atomicAdd(&cnt[mode * K_COUNT + i], loc[i]);
}

// ---------------------------------------------------------------- (c) issue cost
#define R8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define FMAC8 R8(FM)
#define FM(i) asm volatile("v_fmac_f32_e32 %0, %1, %2" : "+v"(f[i]) : "v"(s), "v"(w));
// one chain of six from C = 0 into D[c]; the A operand passes an empty asm so that the chain stays in the loop
#define CH6(c)                                   \
    asm volatile("" : "+v"(a));                  \
    D[c] = MFMA(a, s, z, c);                     \
    D[c] = MFMA(a, w, D[c], c);                  \
    D[c] = MFMA(a, s, D[c], c);                  \
    D[c] = MFMA(a, w, D[c], c);                  \
    D[c] = MFMA(a, s, D[c], c);                  \
    D[c] = MFMA(a, w, D[c], c);
#define SINK(c) asm volatile("" :: "v"(D[c]));
enum { C_FMAC = 0, C_MFMA_INDEP, C_CHAIN1, C_CHAIN2, C_CHAIN4, C_CHAIN1_FMAC56, C_CHAIN1_SPREAD_FMAC56, C_FMAC56, C_FMAC56_DPP24, C_COUNT };
template <int MODE>
__global__ void __launch_bounds__(256) cost_kernel(float *out, int iters) {
    float f[8], s = (float)threadIdx.x * 1e-3f, w = 1.0001f, a = 0.5f;
    for (int i = 0; i < 8; ++i) { f[i] = (float)i; asm volatile("" : "+v"(f[i])); }
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 D[4] = {z, z, z, z};
    for (int it = 0; it < iters; ++it) {
        if (MODE == C_FMAC) {   // 48 independent v_fmac_f32
            FMAC8 FMAC8 FMAC8 FMAC8 FMAC8 FMAC8
        } else if (MODE == C_MFMA_INDEP) {   // 24 MFMAs, four accumulators in turn: each depends on the fourth before it
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                D[0] = MFMA(a, s, D[0], 0); D[1] = MFMA(a, w, D[1], 1); D[2] = MFMA(a, s, D[2], 2); D[3] = MFMA(a, w, D[3], 3);
            }
        } else if (MODE == C_CHAIN1) {   // four chains of six, one after the other
            CH6(0) SINK(0) CH6(1) SINK(1) CH6(2) SINK(2) CH6(3) SINK(3)
        } else if (MODE == C_CHAIN2 || MODE == C_CHAIN4) {   // 24 MFMAs as two / four chains interleaved by the scheduler's choice
            asm volatile("" : "+v"(a));
            constexpr int NC = MODE == C_CHAIN2 ? 2 : 4;
#pragma unroll
            for (int h = 0; h < 4 / NC; ++h) {
#pragma unroll
                for (int c = 0; c < NC; ++c) D[c] = MFMA(a, f[c], z, 0);   // (a B operand of its own per chain: they are four chains to the compiler too)
#pragma unroll
                for (int m = 1; m < 6; ++m)
#pragma unroll
                    for (int c = 0; c < NC; ++c) D[c] = MFMA(a, (m & 1) ? w : f[c], D[c], 0);
#pragma unroll
                for (int c = 0; c < NC; ++c) SINK(c)
                asm volatile("" : "+v"(a));
            }
        } else if (MODE == C_CHAIN1_FMAC56) {   // a group of the forward: one chain of six, then 56 v_fmac_f32 (4 evaluations x 14)
            CH6(0) SINK(0)
            FMAC8 FMAC8 FMAC8 FMAC8 FMAC8 FMAC8 FMAC8
        } else if (MODE == C_CHAIN1_SPREAD_FMAC56) {   // the same with the chain's MFMAs spread over the v_fmac_f32: eight between two of them
            asm volatile("" : "+v"(a));
#define SPREAD(m, b, c) D[0] = MFMA(a, b, c, 0); __builtin_amdgcn_sched_barrier(0); FMAC8 __builtin_amdgcn_sched_barrier(0);
            SPREAD(0, s, z) SPREAD(1, w, D[0]) SPREAD(2, s, D[0]) SPREAD(3, w, D[0]) SPREAD(4, s, D[0]) SPREAD(5, w, D[0])
#undef SPREAD
            SINK(0) FMAC8
        } else if (MODE == C_FMAC56) {
            FMAC8 FMAC8 FMAC8 FMAC8 FMAC8 FMAC8 FMAC8
        } else {   // the parent's group: 56 v_fmac_f32 and 24 v_fmac_f32_dpp
            FMAC8 FMAC8 FMAC8 FMAC8 FMAC8 FMAC8 FMAC8
#define DP(i) asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(f[i]) : "v"(s), "v"(w));
            R8(DP) R8(DP) R8(DP)
#undef DP
        }
    }
    float t = 0.f;
    for (int i = 0; i < 8; ++i) t += f[i];
    for (int c = 0; c < 4; ++c) t += D[c][0] + D[c][1] + D[c][2] + D[c][3];
    out[blockIdx.x * 256 + threadIdx.x] = t;
}
template <int MODE>
static void cost(const char *name, int mfma, int valu, float *out, int wps, bool last) {
    const int iters = 20000, blocks = 256 * wps;
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(cost_kernel<MODE>, dim3(blocks), dim3(256), 0, 0, out, 100);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(cost_kernel<MODE>, dim3(blocks), dim3(256), 0, 0, out, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms = 0.f; hipEventElapsedTime(&ms, e0, e1);
    // every SIMD runs wps waves, each `iters` trips of (mfma + valu) instructions
    const double ns_per_trip_per_simd = ms * 1e6 / ((double)iters * wps);
    printf("  {\"probe\": \"%s\", \"waves_per_simd\": %d, \"mfma_per_trip\": %d, \"valu_per_trip\": %d, \"ms\": %.4f, \"ns_per_trip_per_simd\": %.3f, "
           "\"ns_per_instr_per_simd\": %.4f}%s\n", name, wps, mfma, valu, ms, ns_per_trip_per_simd, ns_per_trip_per_simd / (mfma + valu), last ? "" : ",");
}

int main() {
    printf("{\n");
    // ---- (a)
    float *d_lay, h_lay[2 * 4 * 4 * 64];
    hipMalloc(&d_lay, sizeof(h_lay));
    hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(64), 0, 0, d_lay);
    hipMemcpy(h_lay, d_lay, sizeof(h_lay), hipMemcpyDeviceToHost);
    // expected: D[i] of lane l under abid:t = A of lane 16 (l / 16) + 4 t + i times B of lane l
    int a_ok = 1, b_ok = 1;
    printf(" \"layout\": {\"instruction\": \"v_mfma_f32_4x4x1_16b_f32 cbsz:2 abid:t\", \"a_source_lane\": {\n");
    for (int t = 0; t < 4; ++t) {
        printf("  \"abid%d\": [", t);
        for (int i = 0; i < 4; ++i) {
            printf("[");
            for (int l = 0; l < 64; ++l) {
                const int a_src = (int)h_lay[((0 * 4 + t) * 4 + i) * 64 + l] - 1, b_src = (int)h_lay[((1 * 4 + t) * 4 + i) * 64 + l] - 1;
                a_ok &= a_src == 16 * (l / 16) + 4 * t + i;
                b_ok &= b_src == l;
                printf("%d%s", a_src, l < 63 ? "," : "");
            }
            printf("]%s", i < 3 ? ", " : "");
        }
        printf("]%s\n", t < 3 ? "," : "");
    }
    printf("  },\n  \"a_source_lane_is\": \"a_source_lane[abid t][register i][lane l]\",\n");
    printf("  \"a_is_lane_16_row_plus_4t_plus_i\": %s, \"b_and_d_are_the_lane_itself\": %s},\n", a_ok ? "true" : "false", b_ok ? "true" : "false");

    // ---- (b)
    unsigned long long *d_cnt, h_cnt[M_COUNT * K_COUNT + 1];
    float *d_bad, h_bad[12];
    hipMalloc(&d_cnt, sizeof(h_cnt)); hipMemset(d_cnt, 0, sizeof(h_cnt));
    hipMalloc(&d_bad, sizeof(h_bad)); hipMemset(d_bad, 0, sizeof(h_bad));
    const int blocks_random = 1 << 14, blocks_edge = 1 << 10;   // 2^20 random operand sets (lanes), 2^16 per edge set; x 16 pixels each
    for (int m = 0; m < M_COUNT; ++m)
        hipLaunchKernelGGL(chain_kernel, dim3(m == M_RANDOM ? blocks_random : blocks_edge), dim3(64), 0, 0, d_cnt, d_bad, m, 12345u + 977u * m);
    hipMemcpy(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost);
    hipMemcpy(h_bad, d_bad, sizeof(h_bad), hipMemcpyDeviceToHost);
    static const char *mname[M_COUNT] = {"random", "q0_minus_inf", "nan_and_inf_coefficients", "denormals", "magnitude_1e4_and_more", "q0_plus_minus_zero"};
    unsigned long long other = 0, nanbits = 0;
    printf(" \"chain\": {\"order\": \"(1,q0) (x,qx) (y,qy) (xx,qxx) (xy,qxy) (yy,qyy) from C = 0\", \"reference\": \"power_poly() of blend_power.h\",\n"
           "  \"operand_sets\": {\"random\": %d, \"per_edge_set\": %d, \"pixels_per_set\": 16},\n", blocks_random * 64, blocks_edge * 64);
    for (int m = 0; m < M_COUNT; ++m) {
        const unsigned long long *c = h_cnt + m * K_COUNT;
        other += c[K_OTHER]; nanbits += c[K_NAN_BITS];
        printf("  \"%s\": {\"evaluations\": %llu, \"bit_equal\": %llu, \"zero_of_other_sign\": %llu, \"nan_with_other_bits\": %llu, \"other_mismatch\": %llu},\n",
               mname[m], c[K_TOTAL], c[K_EQUAL], c[K_ZERO_SIGN], c[K_NAN_BITS], c[K_OTHER]);
    }
    if (other)
        printf("  \"first_other_mismatch\": {\"mode\": %d, \"q\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"x\": %g, \"y\": %g, \"power_poly\": %.9g, \"mfma\": %.9g},\n",
               (int)h_bad[0], h_bad[1], h_bad[2], h_bad[3], h_bad[4], h_bad[5], h_bad[6], h_bad[7], h_bad[8], h_bad[9], h_bad[10]);
    printf("  \"chain_reproduced\": %s},\n", (other == 0 && nanbits == 0) ? "true" : "false");

    // ---- (c)
    float *out; hipMalloc(&out, 256 * 8 * 256 * sizeof(float));
    printf(" \"issue_cost\": [\n");
    for (int wps : {1, 6}) {
        cost<C_FMAC>("48 v_fmac_f32", 0, 48, out, wps, false);
        cost<C_MFMA_INDEP>("24 mfma, four accumulators in turn", 24, 0, out, wps, false);
        cost<C_CHAIN1>("24 mfma, dependent chains of six one after the other", 24, 0, out, wps, false);
        cost<C_CHAIN2>("24 mfma, two chains interleaved", 24, 0, out, wps, false);
        cost<C_CHAIN4>("24 mfma, four chains interleaved", 24, 0, out, wps, false);
        cost<C_FMAC56>("56 v_fmac_f32", 0, 56, out, wps, false);
        cost<C_CHAIN1_FMAC56>("chain of six + 56 v_fmac_f32 (a group of the new forward)", 6, 56, out, wps, false);
        cost<C_CHAIN1_SPREAD_FMAC56>("chain of six spread over 56 v_fmac_f32, eight between two MFMAs", 6, 56, out, wps, false);
        cost<C_FMAC56_DPP24>("56 v_fmac_f32 + 24 v_fmac_f32_dpp (a group of the parent)", 0, 80, out, wps, wps == 6);
    }
    const hipError_t e = hipDeviceSynchronize();
    printf(" ],\n \"status\": \"%s\"\n}\n", hipGetErrorString(e));
    return e != hipSuccess;
}
