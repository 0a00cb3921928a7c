// The exponent arithmetic of alpha compositing, shared by every kernel that evaluates a splat on a pixel (blend.hip: the
// forward and every backward; query.hip: compositing at sparse points): one definition, so that their decisions agree
// bit for bit.
#pragma once
#include "common.h"

// The reference skips a splat when power > 0 (src/alpha_blending.cu:93).  power is a negative-semidefinite form -- EWA only
// emits positive-definite conics (cov2d + 0.3 I) -- so it exceeds 0 by rounding only (the expanded polynomial carries ~1e-5 of
// absolute noise in log2 units; at a splat's centre the reference evaluates exp(0) = 1).  No compare per (pixel, splat) is spent
// on it: the raw alpha is exp2 of the polynomial (opacity included, see power_coeffs) with the clamp bit of v_exp_f32 set --
// alpha_raw = min(o exp(power), 1), and a NaN (o < 0, garbage conic) becomes 0 under the DX10 clamp, i.e. "skipped".  Forward
// and every backward kernel share exp2_guard(), so decisions stay reproducible.
// raw alpha = exp2(pw) = o * exp(power); `ok` is always true (kept for the callers' predicate chains)
__device__ __forceinline__ float exp2_guard(float pw, bool &ok) {
    ok = true;
    return __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(pw), 0.f, 1.f);   // folds into v_exp_f32 ... clamp
}

// ---- the splat's exponent: ONE arithmetic for the forward and every backward kernel, so that a pixel's backward
// reproduces its forward's alpha bit for bit (the reference's two kernels share their expression as well,
// src/alpha_blending.cu:78-87 vs :196-203; a decision alpha >= 1/255 that flips between the two passes would corrupt
// the T /= (1 - alpha) replay of that pixel).
//   log2(o) + power(x, y) * log2(e) = q0 + qx x + qy y + qxx x^2 + qxy x y + qyy y^2      x, y: pixel relative to the tile centre
// evaluated as the fused-multiply-add chain q0 -> +x qx -> +y qy -> +xx qxx -> +xy qxy -> +yy qyy.  The matrix-core
// backward gets exactly this chain from two v_mfma_f32_16x16x4_f32 (an f32 MFMA is the ascending fma chain over k
// starting from C: profiles/r02_mfma_fma_chain_probe.json, 2^20 of 2^20 random products bit-equal); the lane = pixel
// kernels run it on the VALU.  The coefficients come from power_coeffs() everywhere (explicit fma, no contraction).
// exp2 of it is the raw alpha o * exp(power) itself.  The reference's "power > 0" guard: see exp2_guard().
#define BLEND_L2E 1.4426950408889634f
struct PowerCoef {
    float q0, qx, qy, qxx, qxy, qyy;
};
// The opacity rides in the constant term: q0 = log2(o) - 0.5 log2(e) c^T Q c, so that exp2 of the polynomial IS o * exp(power)
// (the raw alpha) -- one multiply less per (pixel, splat) evaluation in every kernel.  o <= 0 gives -inf / NaN -> alpha 0
// (the reference: o * G < 1/255 -> skipped).
__device__ __forceinline__ PowerCoef power_coeffs(float u, float v, float cA, float cB, float cC, float o, float cx, float cy) {
#pragma clang fp contract(off)
    const float uc = u - cx, vc = v - cy;  // splat centre relative to the tile centre
    const float tx = __builtin_fmaf(cA, uc, cB * vc);
    const float ty = __builtin_fmaf(cB, uc, cC * vc);
    PowerCoef k;
    k.q0 = __builtin_fmaf(-0.5f * BLEND_L2E, __builtin_fmaf(uc, tx, vc * ty), __builtin_amdgcn_logf(o));
    k.qx = BLEND_L2E * tx;
    k.qy = BLEND_L2E * ty;
    k.qxx = (-0.5f * BLEND_L2E) * cA;
    k.qxy = (-BLEND_L2E) * cB;
    k.qyy = (-0.5f * BLEND_L2E) * cC;
    return k;
}
// lane = pixel evaluation; c0 = [q0 qx qy qxx], c1 = [qxy qyy . .]; x, y, xx = x^2, xy, yy = y^2 exact in f32
__device__ __forceinline__ float power_poly(const float4 &c0, const float4 &c1, float x, float y, float xx, float xy,
                                            float yy) {
    float pw = __builtin_fmaf(x, c0.y, c0.x);
    pw = __builtin_fmaf(y, c0.z, pw);
    pw = __builtin_fmaf(xx, c0.w, pw);
    pw = __builtin_fmaf(xy, c1.x, pw);
    return __builtin_fmaf(yy, c1.y, pw);
}
