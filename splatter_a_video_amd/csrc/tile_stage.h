// Staging of a tile's list for the lane-walk kernels that take the geometry straight from uv / conic / opacity (edit.hip,
// lift.hip): entries in batches of STAGE_SB, thread l of the workgroup fetching entry l one batch ahead (and the ids two ahead), so
// that no global load's latency is waited for between two batches, and parking it in LDS with the exponent coefficients of
// blend_power.h relative to the tile centre and the mask of the 8x8 blocks the splat can reach.
#pragma once
#include "blend_power.h"
#include "common.h"

constexpr int STAGE_SB = 64;   // list entries staged per batch

// What thread l holds of entry l of a batch between its fetch and the moment it is parked in LDS
struct StageFetch {
    float2 u;
    float cA, cB, cC, o;
    float4 col;     // COLOURS: the entry's colour
    int slot;       // !COLOURS: its pair slot
    bool valid;
};

// id of entry q of the tile's list (idx points at its first entry), -1 behind its end (n) and for threads that fetch nothing
__device__ __forceinline__ int stage_load_id(const int *idx, int tid, int q, int n) { return (tid < STAGE_SB && q < n) ? idx[q] : -1; }

// feature [P, 3] (COLOURS) or slots (the tile's first pair slot entry, !COLOURS); the other may be NULL
template <bool COLOURS>
__device__ __forceinline__ StageFetch stage_load(int P, const float2 *uv, const float *conic, const float *opacity, const float *feature,
                                                 const int *slots, int id, int q) {
    StageFetch f;
    f.valid = (unsigned)id < (unsigned)P;   // (an id outside [0, P) becomes an entry that never contributes)
    f.u = make_float2(0.f, 0.f);
    f.cA = f.cB = f.cC = f.o = 0.f;
    f.col = make_float4(0.f, 0.f, 0.f, 0.f);
    f.slot = -1;
    if (f.valid) {
        f.u = uv[id];
        f.cA = conic[3 * (size_t)id];
        f.cB = conic[3 * (size_t)id + 1];
        f.cC = conic[3 * (size_t)id + 2];
        f.o = opacity[id];
        if (COLOURS) f.col = make_float4(feature[3 * (size_t)id], feature[3 * (size_t)id + 1], feature[3 * (size_t)id + 2], 0.f);
        else f.slot = slots[q];
    }
    return f;
}

// threads 0 .. STAGE_SB - 1 of the workgroup park their entry in L (c0: q0 qx qy qxx, c1: qxy qyy . ., mask, and col or slot) with
// the mask of the 8x8 blocks it can reach (the forward's own conservative test: never false for a splat that contributes, so a
// wave that leaves an entry out makes the decisions it would have made -- alpha < 1/255 on all its pixels); an entry that is not
// valid reaches none
template <bool COLOURS, typename LDS>
__device__ __forceinline__ void stage_park(LDS &L, int tid, const StageFetch &f, float tcx, float tcy) {
    if (tid >= STAGE_SB) return;
    float4 k0 = make_float4(-__builtin_inff(), 0.f, 0.f, 0.f), k1 = make_float4(0.f, 0.f, 0.f, 0.f);
    int mask = 0;
    if (f.valid) {
        const PowerCoef k = power_coeffs(f.u.x, f.u.y, f.cA, f.cB, f.cC, f.o, tcx, tcy);
        k0 = make_float4(k.q0, k.qx, k.qy, k.qxx);
        k1 = make_float4(k.qxy, k.qyy, 0.f, 0.f);
        const CullP cp = cull_params(f.cA, f.cB, f.cC, f.o);
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            const float x0 = tcx - 7.5f + (float)(8 * (ww & 1)), y0 = tcy - 7.5f + (float)(8 * (ww >> 1));
            if (cull_test(f.u.x, f.u.y, f.cA, f.cB, f.cC, cp, x0, x0 + 7.f, y0, y0 + 7.f)) mask |= 1 << ww;
        }
    }
    L.c0[tid] = k0;
    L.c1[tid] = k1;
    L.mask[tid] = mask;
    if constexpr (COLOURS) L.col[tid] = f.col;
    else L.slot[tid] = f.slot;
}
