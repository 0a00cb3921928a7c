// Feature lifting (include/splat_hip.h: splat_blend_lift_batch, splat_lift_fold): per-Gaussian features from per-frame 2-D maps.
// With geometry and opacity frozen the composited image is linear in the feature, out[p, c] = sum_g w[p, g] f[g, c] with
// w = alpha * T under the forward's skip and stop rules, and everything a feature fit needs is the transposed operator
//     num[g, c] = sum_frames sum_p pw[p] w[p, g] y[p, c]        den[g] = sum_frames sum_p pw[p] w[p, g]
// -- a front-to-back walk of the tile lists: no replay by division, no dL/dalpha, no geometry terms, no float atomics.
//
// Lanes = list entries, as in blend_bwd_mfma_kernel (blend.hip): lane (n, kk), n = lane & 15 one of 16 entries of the wave's list
// (front first), kk = lane >> 4.  The wave's 8x8 pixel block is walked as four 2x8 strips G; in strip G lane (n, kk) evaluates
// its entry on the pixels m = 4 kk + i (i = 0 .. 3, row-major in the strip).  The pixel reduction is
//     D[channel, entry] += A[channel, pixel] B[pixel, entry]        (v_mfma_f32_16x16x4_f32, K = the four pixels m = 4 kk + i, kk = 0 .. 3)
// with A = pw * y, staged ONCE per wave into operand registers (lane (c, kk) holds channel 16 q + c of its pixels; the weight sum
// rides as one more column, pw itself) and B = the weight the lane has just computed: the product needs no lane movement, and
// the accumulator of lane (n, kk) ends up with channels 16 q + 4 kk .. + 3 of entry n, one 16-byte store.
// The transmittance is the forward's, bit for bit: T in front of entry n is the SEQUENTIAL product T_state (1 - a_0) .. (1 - a_{n-1})
// over the 16-lane DPP row (15 steps of Q = Q[lane - 1] * (1 - a): after step s the lanes 0 .. s hold the forward's value; a tree
// scan would round differently and flip stop decisions).  A product by a factor <= 1 never grows, so "the pixel stopped at or
// before entry n" is Q_n < 1e-4 of the products taken as if nothing stopped.
#include "blend_power.h"
#include "common.h"
#include "tile_stage.h"

namespace {

constexpr int LIFT_SB = STAGE_SB;   // list entries staged per batch (tile_stage.h): thread l of the workgroup fetches entry l
typedef float lift_f32x4 __attribute__((ext_vector_type(4)));

struct LiftArgs {
    int F, P, D, c0, cn, want_den;
    const float2 *uv;
    const float *conic, *opacity;
    long long op_fs;
    const int *idx_sorted;
    const int2 *tile_range;
    const int *slot_sorted;
    long long cap;
    int W, H, gx, T;
    const float *maps, *pixel_weight;
    float *pair_sums;
    int NQ;   // record stride in 16-byte chunks
};

template <int NB>
struct LiftLDS {
    static constexpr int RS = 16 * NB + 4;   // floats per partial record (+ 4: consecutive entries start in different banks)
    float4 c0[LIFT_SB + 1];    // q0 qx qy qxx; entry LIFT_SB is inert (q0 = log2(0)): the padding of a wave's group of 16
    float4 c1[LIFT_SB + 1];    // qxy qyy . .
    int slot[LIFT_SB];
    int mask[LIFT_SB];         // bit w: the splat can reach alpha >= 1/255 on a pixel of wave w's 8x8 block (cull_test, common.h)
    unsigned short list[4][LIFT_SB + 16];   // wave w's entries of the batch, list order, padded with the inert entry
    unsigned long long wrote[4];            // bit e: wave w has written part[w][e]
    alignas(16) float part[4][LIFT_SB][RS];
};

// value of the previous lane of the 16-lane row; lane 0 of a row gets `first`
__device__ __forceinline__ float row_prev(float first, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, first), __builtin_bit_cast(int, v), 0x111,
                                                                 0xf, 0xf, false));   // row_shr:1
}

// one of the lane's 16 pixels is neither finished nor outside (T_state < 0: finished, outside the image or of weight 0)
__device__ __forceinline__ bool lift_alive(const float (&Ts)[4][4]) {
    bool alive = false;
#pragma unroll
    for (int G = 0; G < 4; ++G)
#pragma unroll
        for (int i = 0; i < 4; ++i) alive = alive || Ts[G][i] >= 0.f;
    return alive;
}

template <int NB>
__global__ void __launch_bounds__(256)
blend_lift_kernel(const LiftArgs A) {
    __shared__ LiftLDS<NB> L;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n16 = lane & 15, kk = lane >> 4;
    const int f = (int)(blockIdx.x / (unsigned)A.T), tile = (int)(blockIdx.x - (unsigned)f * (unsigned)A.T);
    const int tx = tile % A.gx, ty = tile / A.gx;
    const float tcx = (float)(tx * TILE) + 7.5f, tcy = (float)(ty * TILE) + 7.5f;
    const int2 range = A.tile_range[(size_t)f * A.T + tile];
    const int beg = imax_(range.x, 0);
    const int n = imax_((int)(A.cap < (long long)range.y ? A.cap : (long long)range.y) - beg, 0);
    if (n == 0) return;   // (the whole workgroup)
    const int *idx = A.idx_sorted + (size_t)f * (size_t)A.cap + beg, *slots = A.slot_sorted + (size_t)f * (size_t)A.cap + beg;
    const float2 *uv = A.uv + (size_t)f * A.P;
    const float *conic = A.conic + (size_t)f * 3 * A.P, *opacity = A.opacity + (size_t)f * (size_t)A.op_fs;
    float4 *rec = reinterpret_cast<float4 *>(A.pair_sums) + (size_t)f * (size_t)A.cap * A.NQ;

    // ---- the wave's window of pw * y as A operands, and the pixels' transmittance; pixel (G, i) of this lane is
    //      (bx + i, by + 2 G) of the tile
    const int bx = (w & 1) * 8 + 4 * (kk & 1), by = (w >> 1) * 8 + (kk >> 1);
    float yop[4][4][NB], Ts[4][4];
    {
        const size_t HW = (size_t)A.H * A.W;
        const float *pwm = A.pixel_weight ? A.pixel_weight + (size_t)f * HW : nullptr;
        const float *maps = A.maps + ((size_t)f * A.D + A.c0) * HW;
#pragma unroll
        for (int G = 0; G < 4; ++G) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int px = tx * TILE + bx + i, py = ty * TILE + by + 2 * G;
                const bool inside = px < A.W && py < A.H;
                const size_t pix = (size_t)A.W * py + px;
                const float pw = inside ? (pwm ? pwm[pix] : 1.f) : 0.f;
                const bool live = pw != 0.f;   // a pixel of weight 0 contributes exactly 0, whatever its map holds: selected
                Ts[G][i] = live ? 1.f : -1.f;
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    const int col = 16 * q + n16;
                    float v = 0.f;
                    if (live && col < A.cn) v = pw * maps[(size_t)col * HW + pix];
                    else if (live && col == A.cn && A.want_den) v = pw;
                    yop[G][i][q] = v;
                }
            }
        }
    }
    float xs[4], ys[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        xs[i] = (float)(bx + i) - 7.5f;       // relative to the tile centre, as in blend.hip
        ys[i] = (float)(by + 2 * i) - 7.5f;   // (of strip G = i)
    }
    if (tid == 0) {   // the inert entry
        L.c0[LIFT_SB] = make_float4(-__builtin_inff(), 0.f, 0.f, 0.f);
        L.c1[LIFT_SB] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    int id = stage_load_id(idx, tid, tid, n);
    StageFetch pay = stage_load<false>(A.P, uv, conic, opacity, nullptr, slots, id, tid);
    id = stage_load_id(idx, tid, LIFT_SB + tid, n);
    int done_to = 0;   // entries [0, done_to) have their record
    bool alive = lift_alive(Ts);
    for (int base = 0; base < n; base += LIFT_SB) {
        const int nb = imin_(LIFT_SB, n - base);
        stage_park<false>(L, tid, pay, tcx, tcy);
        __syncthreads();
        pay = stage_load<false>(A.P, uv, conic, opacity, nullptr, slots, id, base + LIFT_SB + tid);   // the next batch, in flight during this one's walk
        id = stage_load_id(idx, tid, base + 2 * LIFT_SB + tid, n);
        unsigned long long wrote = 0ull;
        if (__ballot(alive) != 0ull) {
            // the wave's entries of the batch, in list order
            const bool keep = (L.mask[lane] >> w) & 1;
            const unsigned long long m = __ballot(keep);
            const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            const int cnt = __popcll(m);
            if (keep) L.list[w][before] = (unsigned short)lane;
            if (lane < 16) L.list[w][cnt + lane] = (unsigned short)LIFT_SB;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            wrote = m;
            for (int j0 = 0; j0 < cnt; j0 += 16) {
                const int e = L.list[w][j0 + n16];
                const float4 c0 = L.c0[e], c1 = L.c1[e];
                lift_f32x4 acc[NB];
#pragma unroll
                for (int q = 0; q < NB; ++q) acc[q] = lift_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int G = 0; G < 4; ++G) {
                    float al[4], fac[4], Q[4], wgt[4];
                    bool any = false;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        bool ok;
                        const float x = xs[i], y = ys[G];
                        const float a = fminf(0.99f, exp2_guard(power_poly(c0, c1, x, y, x * x, x * y, y * y), ok));
                        al[i] = (ok && !(a < (1.0f / 255.0f))) ? a : 0.f;
                        any = any || al[i] != 0.f;
                        fac[i] = 1.f - al[i];
                        Q[i] = Ts[G][i] * fac[i];   // (lane 0 of the row: final)
                    }
                    if (__ballot(any) == 0ull) continue;   // nobody applies on the strip: every pixel keeps its state
#pragma unroll
                    for (int s = 1; s < 16; ++s) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float t = dpp_f<0x111, 0xf, 0xf, true>(Q[i]) * fac[i];   // row_shr:1 (one v_mul_f32_dpp)
                            Q[i] = n16 == 0 ? Q[i] : t;
                        }
                    }
                    any = false;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float Tfront = row_prev(Ts[G][i], Q[i]);
                        wgt[i] = (Q[i] < 0.0001f) ? 0.f : al[i] * Tfront;
                        any = any || wgt[i] != 0.f;
                        const float last = dpp_f<0x15f, 0xf, 0xf, true>(Q[i]);   // row_newbcast:15
                        Ts[G][i] = (last < 0.0001f) ? -1.f : last;
                    }
                    if (__ballot(any) == 0ull) continue;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < NB; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(yop[G][i][q], wgt[i], acc[q], 0, 0, 0);
                }
                if (e < LIFT_SB) {
#pragma unroll
                    for (int q = 0; q < NB; ++q)
                        *reinterpret_cast<float4 *>(&L.part[w][e][16 * q + 4 * kk]) = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
                }
            }
        }
        if (lane == 0) L.wrote[w] = wrote;
        __syncthreads();
        // the four waves' partials in the order 0 .. 3; a wave that left the entry out holds nothing of it
        {
            const unsigned long long m0 = L.wrote[0], m1 = L.wrote[1], m2 = L.wrote[2], m3 = L.wrote[3];
            for (int i = tid; i < nb * A.NQ; i += 256) {
                const int ql = i / A.NQ, c4 = i - ql * A.NQ;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                auto add = [&](int ww) {
                    const float4 b = *reinterpret_cast<const float4 *>(&L.part[ww][ql][4 * c4]);
                    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
                };
                if ((m0 >> ql) & 1ull) add(0);
                if ((m1 >> ql) & 1ull) add(1);
                if ((m2 >> ql) & 1ull) add(2);
                if ((m3 >> ql) & 1ull) add(3);
                const int slot = L.slot[ql];
                if (slot >= 0 && (long long)slot < A.cap) rec[(size_t)slot * A.NQ + c4] = v;
            }
        }
        done_to = base + nb;
        alive = lift_alive(Ts);
        if (__syncthreads_and(!alive)) break;   // every pixel of the tile is finished
    }
    // behind the last batch walked nothing applies on any pixel: zeros (the fold reads every slot)
    for (int i = done_to * A.NQ + tid; i < n * A.NQ; i += 256) {
        const int ql = i / A.NQ, c4 = i - ql * A.NQ;
        const int slot = slots[ql];
        if (slot >= 0 && (long long)slot < A.cap) rec[(size_t)slot * A.NQ + c4] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Per Gaussian the sum of its records -- slots [goff[f, i-1], goff[f, i]) in ascending order into the frame's sum, the frames'
// sums in ascending order onto what num / den hold: NQ neighbouring lanes own one Gaussian, lane q the 16-byte chunk q of every
// one of its records (part (b) of frames_wide_fold_kernel, frames.hip).
struct LiftFoldArgs {
    int F, P, cn, want_den, NQ, c0;
    long long cap, nstride;
    const int *goff;
    const float4 *recs;
    float *num, *den;
};

constexpr int LIFT_FOLD_U = 4;   // records a lane requests together

__global__ void __launch_bounds__(256)
lift_fold_kernel(const LiftFoldArgs A) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / A.NQ), q = (int)(t - (long long)i * A.NQ);
    if (i >= A.P) return;
    float *d = A.num + (size_t)i * (size_t)A.nstride + A.c0;
    float a4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * q + j;
        a4[j] = k < A.cn ? d[k] : (k == A.cn && A.want_den) ? A.den[i] : 0.f;
    }
    for (int f = 0; f < A.F; ++f) {
        const int *goff = A.goff + (size_t)f * A.P;
        long long b = i > 0 ? goff[i - 1] : 0, e = goff[i];
        if (e > A.cap) e = A.cap;   // a frame that outgrew the capacity dropped its surplus pairs
        if (b < 0) b = 0;
        const float4 *recs = A.recs + (size_t)f * (size_t)A.cap * A.NQ + q;
        float4 fs = make_float4(0.f, 0.f, 0.f, 0.f);
        for (long long s = b; s < e; s += LIFT_FOLD_U) {
            float4 v[LIFT_FOLD_U];
#pragma unroll
            for (int u = 0; u < LIFT_FOLD_U; ++u)
                v[u] = s + u < e ? recs[(size_t)(s + u) * A.NQ] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < LIFT_FOLD_U; ++u) {
                if (s + u >= e) break;
                fs.x += v[u].x; fs.y += v[u].y; fs.z += v[u].z; fs.w += v[u].w;
            }
        }
        a4[0] += fs.x; a4[1] += fs.y; a4[2] += fs.z; a4[3] += fs.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * q + j;
        if (k < A.cn) d[k] = a4[j];
        else if (k == A.cn && A.want_den) A.den[i] = a4[j];
    }
}

}  // namespace

extern "C" size_t splat_lift_pair_stride(int cn, int want_den) {
    if (cn < 1 || cn > 32) return 0;
    return (size_t)((cn + (want_den ? 1 : 0) + 3) & ~3);
}

extern "C" int splat_blend_lift_batch(int F, int P, int D, int c0, int cn, const float *uv, const float *conic, const float *opacity,
                                      int64_t opacity_frame_stride, const int32_t *idx_sorted, const int32_t *tile_range,
                                      const int32_t *slot_sorted, int64_t capacity, int W, int H, const float *maps,
                                      const float *pixel_weight, int want_den, float *pair_sums, splat_stream_t stream) {
    SPLAT_CHECK_ARG(F >= 1 && P >= 1 && D >= 1 && W >= 1 && H >= 1 && capacity >= 1 && opacity_frame_stride >= 0, "bad sizes");
    SPLAT_CHECK_ARG(c0 >= 0 && cn >= 1 && cn <= 32 && (long long)c0 + cn <= D, "the chunk must be 1..32 channels inside the maps");
    const long long gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    SPLAT_CHECK_ARG((long long)F * gx * gy < (1ll << 31) && capacity <= 0x7fffffffll, "too many tiles or pairs");
    SPLAT_CHECK_ARG(uv && conic && opacity && idx_sorted && tile_range && slot_sorted && maps && pair_sums, "null pointer");
    SPLAT_CHECK_ARG((uintptr_t)pair_sums % 16 == 0, "pair_sums must be 16-byte aligned");
    LiftArgs A;
    memset(&A, 0, sizeof(A));
    A.F = F; A.P = P; A.D = D; A.c0 = c0; A.cn = cn; A.want_den = want_den ? 1 : 0;
    A.uv = (const float2 *)uv; A.conic = conic; A.opacity = opacity; A.op_fs = opacity_frame_stride;
    A.idx_sorted = idx_sorted; A.tile_range = (const int2 *)tile_range; A.slot_sorted = slot_sorted;
    A.cap = capacity; A.W = W; A.H = H; A.gx = (int)gx; A.T = (int)(gx * gy);
    A.maps = maps; A.pixel_weight = pixel_weight; A.pair_sums = pair_sums;
    A.NQ = (int)splat_lift_pair_stride(cn, want_den) / 4;
    const dim3 grid((unsigned)((long long)F * A.T));
    const int cols = cn + A.want_den;   // 16 columns per accumulator
    if (cols <= 16) SPLAT_LAUNCH("blend_lift", blend_lift_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, A);
    else if (cols <= 32) SPLAT_LAUNCH("blend_lift", blend_lift_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, A);
    else SPLAT_LAUNCH("blend_lift", blend_lift_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, A);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_lift_fold(int F, int P, int cn, int want_den, int64_t capacity, const int32_t *goff_incl, const float *pair_sums,
                               float *num, int64_t num_stride, int c0, float *den, splat_stream_t stream) {
    SPLAT_CHECK_ARG(F >= 1 && P >= 1 && capacity >= 1, "bad sizes");
    SPLAT_CHECK_ARG(c0 >= 0 && cn >= 1 && cn <= 32 && num_stride >= (int64_t)c0 + cn, "the chunk must be 1..32 channels inside num");
    SPLAT_CHECK_ARG(goff_incl && pair_sums && num && (den || !want_den), "null pointer");
    SPLAT_CHECK_ARG((uintptr_t)pair_sums % 16 == 0, "pair_sums must be 16-byte aligned");
    LiftFoldArgs A;
    memset(&A, 0, sizeof(A));
    A.F = F; A.P = P; A.cn = cn; A.want_den = want_den ? 1 : 0; A.c0 = c0;
    A.NQ = (int)splat_lift_pair_stride(cn, want_den) / 4;
    A.cap = capacity; A.nstride = num_stride;
    A.goff = goff_incl; A.recs = (const float4 *)pair_sums; A.num = num; A.den = den;
    const long long threads = (long long)P * A.NQ;
    SPLAT_CHECK_ARG((threads + 255) / 256 < (1ll << 31), "bad sizes (too many Gaussians)");
    SPLAT_LAUNCH("lift_fold", lift_fold_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}
