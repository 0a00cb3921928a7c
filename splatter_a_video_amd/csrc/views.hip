// Display-ready frames of the novel-view / stereo clips (include/splat_hip_views.h): float images [F,3,H,W] -> bytes [F,H,W,3].
// One image: the reference's (x.clamp(0, 1) * 255).astype(np.uint8) (src/trainer_fragGS.py:1147-1150).  Two images: the
// anaglyph mix of get_stereo_rendered_imgs (:1250-1253) -- the reference mixes in float64; this kernel pins float32 with
// every product and sum rounded once (no contraction), so that a numpy float32 restatement gives the same bytes.
// Bandwidth bound (12 or 24 B in, 3 B out per pixel): a thread takes four consecutive pixels of a frame -- one 16-byte load
// per plane, three 4-byte stores -- and the last H*W % 4 pixels of every frame go one per thread.  No LDS, no atomics.
#include "common.h"
#include "../../include/splat_hip_views.h"

namespace {

constexpr int PRESENT_BLOCK = 256;

struct PresentMix {
    float m[18];
};

// planes of H*W floats start on a 16-byte boundary only when H*W % 4 == 0 (and byte rows of 3*H*W on a 4-byte one)
struct __attribute__((packed, aligned(4))) Float4U {
    float v[4];
};
struct __attribute__((packed, aligned(1))) WordU {
    uint32_t v;
};

__device__ __forceinline__ float unit_clamp(float x) {
    const float v = x > 0.f ? x : 0.f;  // (NaN compares false: 0)
    return v < 1.f ? v : 1.f;
}

__device__ __forceinline__ uint32_t unit_byte(float v) {
#pragma clang fp contract(off)
    return (uint32_t)(int)(v * 255.0f);
}

__device__ __forceinline__ uint32_t mix_byte(const float *m, const float l[3], const float r[3]) {
#pragma clang fp contract(off)
    float o = m[0] * l[0];
    o = o + m[1] * l[1];
    o = o + m[2] * l[2];
    o = o + m[3] * r[0];
    o = o + m[4] * r[1];
    o = o + m[5] * r[2];
    float s = o * 255.0f;
    s = s > 0.f ? s : 0.f;
    s = s < 255.f ? s : 255.f;
    return (uint32_t)(int)s;
}

template <bool ALIGNED>
__device__ __forceinline__ void load4(const float *p, float v[4]) {
    if (ALIGNED) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const Float4U q = *reinterpret_cast<const Float4U *>(p);
        v[0] = q.v[0]; v[1] = q.v[1]; v[2] = q.v[2]; v[3] = q.v[3];
    }
}

// the three bytes of one pixel from its clamped channels
template <bool STEREO>
__device__ __forceinline__ void pixel_bytes(const PresentMix &mix, const float l[3], const float r[3], uint32_t o[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = STEREO ? mix_byte(mix.m + 6 * c, l, r) : unit_byte(l[c]);
}

template <bool STEREO, bool ALIGNED>
__global__ void __launch_bounds__(PRESENT_BLOCK)
frames_present_kernel(int HW, const float *__restrict__ a, const float *__restrict__ b, PresentMix mix,
                      uint8_t *__restrict__ out) {
    const int quads = HW >> 2, tail = HW & 3;
    const int t = blockIdx.x * PRESENT_BLOCK + threadIdx.x;
    if (t >= quads + tail) return;
    const size_t f = blockIdx.y;
    const float *pa = a + f * 3 * (size_t)HW;
    const float *pb = STEREO ? b + f * 3 * (size_t)HW : nullptr;
    uint8_t *po = out + f * 3 * (size_t)HW;
    if (t >= quads) {  // one of the last H*W % 4 pixels
        const int p = 4 * quads + (t - quads);
        float l[3], r[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            l[c] = unit_clamp(pa[(size_t)c * HW + p]);
            if (STEREO) r[c] = unit_clamp(pb[(size_t)c * HW + p]);
        }
        uint32_t o[3];
        pixel_bytes<STEREO>(mix, l, r, o);
        po[3 * (size_t)p] = (uint8_t)o[0]; po[3 * (size_t)p + 1] = (uint8_t)o[1]; po[3 * (size_t)p + 2] = (uint8_t)o[2];
        return;
    }
    const int p0 = 4 * t;
    float la[3][4], ra[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        load4<ALIGNED>(pa + (size_t)c * HW + p0, la[c]);
        if (STEREO) load4<ALIGNED>(pb + (size_t)c * HW + p0, ra[c]);
    }
    uint32_t bytes[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float l[3], r[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            l[c] = unit_clamp(la[c][k]);
            if (STEREO) r[c] = unit_clamp(ra[c][k]);
        }
        pixel_bytes<STEREO>(mix, l, r, bytes + 3 * k);
    }
    uint8_t *q = po + 3 * (size_t)p0;  // 12 bytes: three words
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        const uint32_t word = bytes[4 * w] | (bytes[4 * w + 1] << 8) | (bytes[4 * w + 2] << 16) | (bytes[4 * w + 3] << 24);
        if (ALIGNED) reinterpret_cast<uint32_t *>(q)[w] = word;
        else reinterpret_cast<WordU *>(q)[w].v = word;
    }
}

template <bool STEREO>
void launch_present(bool aligned, dim3 grid, hipStream_t s, int HW, const float *a, const float *b, const PresentMix &mix,
                    uint8_t *out) {
    if (aligned)
        SPLAT_LAUNCH("frames_present", (frames_present_kernel<STEREO, true>), grid, dim3(PRESENT_BLOCK), 0, s, HW, a, b, mix, out);
    else
        SPLAT_LAUNCH("frames_present", (frames_present_kernel<STEREO, false>), grid, dim3(PRESENT_BLOCK), 0, s, HW, a, b, mix, out);
}

}  // namespace

extern "C" int splat_views_abi_version(void) { return SPLAT_VIEWS_ABI_VERSION; }

extern "C" int splat_frames_present(int F, int H, int W, const float *a, const float *b, const float *mix_host, uint8_t *out,
                                    void *stream) {
    SPLAT_CHECK_ARG(F >= 1 && F <= 65535, "bad sizes (1 <= F <= 65535)");
    SPLAT_CHECK_ARG(H > 0 && W > 0 && (long long)H * W <= 0x7fffffffll / 3, "bad sizes (H * W must be positive, 3 * H * W below 2^31)");
    SPLAT_CHECK_ARG(a && out, "null pointer");
    SPLAT_CHECK_ARG(!b || mix_host, "two images need the 3 x 6 mix matrix (mix_host)");
    const int HW = H * W;
    PresentMix mix;
    memset(&mix, 0, sizeof(mix));
    if (b) memcpy(mix.m, mix_host, sizeof(mix.m));
    const bool aligned = (HW & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && ((uintptr_t)out & 3) == 0;
    const dim3 grid((unsigned)(((HW >> 2) + (HW & 3) + PRESENT_BLOCK - 1) / PRESENT_BLOCK), (unsigned)F);
    if (b) launch_present<true>(aligned, grid, (hipStream_t)stream, HW, a, b, mix, out);
    else launch_present<false>(aligned, grid, (hipStream_t)stream, HW, a, b, mix, out);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}
