// Appearance editing (include/splat_hip.h: splat_blend_fit_color, splat_tile_loss_sum): the colours of frozen geometry fitted to
// an edited frame -- the reference's optimize_appearance_from_mask / _from_img (src/trainer_fragGS.py:999-1120), which run the
// whole renderer and its whole backward a thousand times for tensors that are frozen.  With geometry and opacity fixed every
// weight alpha * T is a constant, the image is linear in the colours, and one launch per iteration does what is left: composite a
// tile, form the MSE residual against the edited frame, reduce dL/dcolour of every list entry over the tile's pixels.  No image
// and no gradient image go through memory; no dL/dalpha, no replay by division, no geometry terms; no float atomics.
#include "blend_power.h"
#include "common.h"
#include "tile_stage.h"

namespace {

constexpr int FIT_SB = STAGE_SB;   // list entries staged per batch (tile_stage.h): lane l of wave 0 fetches entry l

struct FitArgs {
    int P;
    const float2 *uv;
    const float *conic, *opacity, *feature;
    const int *idx_sorted;
    const int2 *tile_range;
    const int *slot_sorted;
    long long capacity;
    float bg;
    int W, H, gx, T;
    const float *target, *pixel_weight;
    const int *active_tiles;
    float *tile_loss;
    float4 *pair_grad;
    float *out;
    int *ncontrib;
    float inv_n;   // 1 / (3 H W)
};

struct FitLDS {
    float4 c0[FIT_SB + 1];    // q0 qx qy qxx; entry FIT_SB is inert (q0 = log2(0)): the padding of a wave's group of four
    float4 c1[FIT_SB + 1];    // qxy qyy . .
    float4 col[FIT_SB + 1];   // r g b .
    int slot[FIT_SB];
    int mask[FIT_SB];         // bit w: the splat can reach alpha >= 1/255 on a pixel of wave w's 8x8 block (cull_test, common.h)
    float4 part[16][FIT_SB + 1];  // pass 2: an entry's sums over the 16 DPP rows of the tile (row 4 w + r = lanes 16 r .. 16 r + 15 of wave w)
    float red[4];
    int last[4];
};

// One evaluation of the forward (blend.hip, blend_fwd_kernel): the weight alpha * T of the splat on this pixel, 0 where it is
// skipped (alpha < 1/255) or the pixel stops; T < 0: the pixel is finished, |T| its final transmittance.
__device__ __forceinline__ float fit_weight(const float4 &c0, const float4 &c1, float x, float y, float xx, float xy, float yy, float &T) {
    bool ok;
    const float a = fminf(0.99f, exp2_guard(power_poly(c0, c1, x, y, xx, xy, yy), ok));
    const float alpha = (ok && !(a < (1.0f / 255.0f))) ? a : 0.f;
    const float nT = T * (1.f - alpha);
    const bool sat = nT < 0.0001f;
    const float wgt = sat ? 0.f : alpha * T;
    T = sat ? -fabsf(T) : nT;
    return wgt;
}

// sum over the 16 lanes of every DPP row; the row's total lands in its lane 15
__device__ __forceinline__ float row_sum_to_lane15(float v) {
    v += dpp_f<0x111, 0xf, 0xf, true>(v);  // row_shr:1
    v += dpp_f<0x112, 0xf, 0xf, true>(v);  // row_shr:2
    v += dpp_f<0x114, 0xf, 0xf, true>(v);  // row_shr:4
    v += dpp_f<0x118, 0xf, 0xf, true>(v);  // row_shr:8
    return v;
}

__global__ void __launch_bounds__(256)
blend_fit_color_kernel(const FitArgs A) {
    __shared__ FitLDS L;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tile = A.active_tiles ? A.active_tiles[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)tile >= (unsigned)A.T) return;   // (the whole workgroup)
    const int tx = tile % A.gx, ty = tile / A.gx;
    // lane = pixel; a wave is one 8x8 block of the tile (a splat that misses the block costs its wave no reduction)
    const int lx = (w & 1) * 8 + (lane & 7), ly = (w >> 1) * 8 + (lane >> 3);
    const int px = tx * TILE + lx, py = ty * TILE + ly;
    const float x = (float)lx - 7.5f, y = (float)ly - 7.5f;   // relative to the tile centre, as in blend.hip
    const float xx = x * x, xy = x * y, yy = y * y;
    const float tcx = (float)(tx * TILE) + 7.5f, tcy = (float)(ty * TILE) + 7.5f;
    const bool inside = px < A.W && py < A.H;
    const int2 range = A.tile_range[tile];
    const int beg = imax_(range.x, 0);
    const int n = imax_((int)(A.capacity < (long long)range.y ? A.capacity : (long long)range.y) - beg, 0);
    const int *idx = A.idx_sorted + beg, *slots = A.slot_sorted + beg;   // the tile's list

    if (tid == 0) {   // the inert entry
        L.c0[FIT_SB] = make_float4(-__builtin_inff(), 0.f, 0.f, 0.f);
        L.c1[FIT_SB] = make_float4(0.f, 0.f, 0.f, 0.f);
        L.col[FIT_SB] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- pass 1: the forward.  A wave walks the entries of a batch that can reach its block, four at a time, straight from the
    // ballot of their mask bits (wave-uniform: scalar registers)
    float T = inside ? 1.f : -1.f, F0 = 0.f, F1 = 0.f, F2 = 0.f;
    int last = 0;
    {
        int id = stage_load_id(idx, tid, tid, n);
        StageFetch pay = stage_load<true>(A.P, A.uv, A.conic, A.opacity, A.feature, slots, id, tid);
        id = stage_load_id(idx, tid, FIT_SB + tid, n);
        for (int base = 0; base < n; base += FIT_SB) {
            stage_park<true>(L, tid, pay, tcx, tcy);
            __syncthreads();
            pay = stage_load<true>(A.P, A.uv, A.conic, A.opacity, A.feature, slots, id, base + FIT_SB + tid);   // the next batch, in flight during this one's walk
            id = stage_load_id(idx, tid, base + 2 * FIT_SB + tid, n);
            if (__ballot(T >= 0.f) != 0ull) {
                unsigned long long m = __ballot((L.mask[lane] >> w) & 1);
                while (m) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int e = m ? (int)__builtin_ctzll(m) : FIT_SB;
                        m &= m - 1ull;
                        const float4 col = L.col[e];
                        const float wgt = fit_weight(L.c0[e], L.c1[e], x, y, xx, xy, yy, T);
                        F0 = __builtin_fmaf(col.x, wgt, F0);
                        F1 = __builtin_fmaf(col.y, wgt, F1);
                        F2 = __builtin_fmaf(col.z, wgt, F2);
                        last = wgt > 0.f ? base + e + 1 : last;
                    }
                }
            }
            if (__syncthreads_and(T < 0.f)) break;   // every pixel of the tile is finished
        }
    }
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, term = 0.f;
    if (inside) {
        const size_t HW = (size_t)A.H * A.W, pix = (size_t)A.W * py + px;
        const float Tf = fabsf(T);
        const float o0 = F0 + Tf * A.bg, o1 = F1 + Tf * A.bg, o2 = F2 + Tf * A.bg;
        if (A.out) {
            A.out[pix] = o0;
            A.out[HW + pix] = o1;
            A.out[2 * HW + pix] = o2;
        }
        if (A.ncontrib) A.ncontrib[pix] = last;
        const float pw = (A.pixel_weight ? A.pixel_weight[pix] : 1.f) * A.inv_n;
        const float d0 = o0 - A.target[3 * pix], d1 = o1 - A.target[3 * pix + 1], d2 = o2 - A.target[3 * pix + 2];
        r0 = 2.f * pw * d0;
        r1 = 2.f * pw * d1;
        r2 = 2.f * pw * d2;
        term = pw * (d0 * d0 + d1 * d1 + d2 * d2);
    }
    term = wave_sum_to_lane63(term);
    last = wave_max_i(last);
    if (lane == 63) {
        L.red[w] = term;
        L.last[w] = last;
    }
    __syncthreads();
    if (tid == 0) A.tile_loss[tile] = ((L.red[0] + L.red[1]) + L.red[2]) + L.red[3];
    const int nproc = imax_(imax_(L.last[0], L.last[1]), imax_(L.last[2], L.last[3]));   // the tile's largest last contributor

    // ---- pass 2: the same walk, the same decisions; per entry sum_p w_p r_pc over the 256 pixels: DPP sums over the 16 lanes of
    // a row, the 16 row sums of the tile through LDS, added in a fixed order by the lane that stores the entry's record
    T = inside ? 1.f : -1.f;
    {
        int id = stage_load_id(idx, tid, tid, nproc);
        StageFetch pay = stage_load<false>(A.P, A.uv, A.conic, A.opacity, A.feature, slots, id, tid);
        id = stage_load_id(idx, tid, FIT_SB + tid, nproc);
        const int prow = 4 * w + (lane >> 4);
        for (int base = 0; base < nproc; base += FIT_SB) {
            const int nb = imin_(FIT_SB, nproc - base);
            stage_park<false>(L, tid, pay, tcx, tcy);
            __syncthreads();
            pay = stage_load<false>(A.P, A.uv, A.conic, A.opacity, A.feature, slots, id, base + FIT_SB + tid);
            id = stage_load_id(idx, tid, base + 2 * FIT_SB + tid, nproc);
            unsigned long long m = __ballot((L.mask[lane] >> w) & 1);
            while (m) {
                float wg[4], g[4][3];
                int e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    e[u] = m ? (int)__builtin_ctzll(m) : FIT_SB;
                    m &= m - 1ull;
                    wg[u] = fit_weight(L.c0[e[u]], L.c1[e[u]], x, y, xx, xy, yy, T);
                    g[u][0] = g[u][1] = g[u][2] = 0.f;
                }
                // wave-uniform: one of the four splats applies on a pixel of this wave's block
                if (__ballot((wg[0] != 0.f) | (wg[1] != 0.f) | (wg[2] != 0.f) | (wg[3] != 0.f)) != 0ull) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        g[u][0] = row_sum_to_lane15(wg[u] * r0);
                        g[u][1] = row_sum_to_lane15(wg[u] * r1);
                        g[u][2] = row_sum_to_lane15(wg[u] * r2);
                    }
                }
                if ((lane & 15) == 15) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) L.part[prow][e[u]] = make_float4(g[u][0], g[u][1], g[u][2], 0.f);
                }
            }
            __syncthreads();
            if (tid < nb) {
                // rows 0 .. 15 in ascending order; the rows of a wave that left the entry out hold nothing of it
                const int reach = L.mask[tid];
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if ((reach >> (r >> 2)) & 1) {
                        const float4 b = L.part[r][tid];
                        a.x += b.x;
                        a.y += b.y;
                        a.z += b.z;
                    }
                }
                const int slot = L.slot[tid];
                if (slot >= 0 && (long long)slot < A.capacity) A.pair_grad[slot] = make_float4(a.x, a.y, a.z, 0.f);
            }
            __syncthreads();
        }
    }
    // behind the last contributor nothing applies on any pixel: zeros (the segment sum reads every slot)
    for (int q = nproc + tid; q < n; q += 256) {
        const int slot = A.slot_sorted[beg + q];
        if (slot >= 0 && (long long)slot < A.capacity) A.pair_grad[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// history[slot] = sum of the T tile partials: thread t adds tiles t, t + 256, .. in ascending order, then a fixed tree over the
// 256 partial sums
__global__ void __launch_bounds__(256)
tile_loss_sum_kernel(int T, const float *__restrict__ tile_loss, float *__restrict__ dst) {
    __shared__ float s[256];
    const int tid = threadIdx.x;
    float a = 0.f;
    for (int i = tid; i < T; i += 256) a += tile_loss[i];
    s[tid] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s[tid] += s[tid + h];
        __syncthreads();
    }
    if (tid == 0) *dst = s[0];
}

}  // namespace

extern "C" int splat_blend_fit_color(int P, int C, const float *uv, const float *conic, const float *opacity, const float *feature,
                                     const int32_t *idx_sorted, const int32_t *tile_range, const int32_t *slot_sorted,
                                     int64_t capacity, float bg, int W, int H, const float *target, const float *pixel_weight,
                                     int n_active, const int32_t *active_tiles, float *tile_loss, float *pair_grad, float *out,
                                     int32_t *ncontrib, splat_stream_t stream) {
    SPLAT_CHECK_ARG(C == 3, "C must be 3 (feature [P, 3], target [H, W, 3])");
    SPLAT_CHECK_ARG(P >= 1 && W >= 1 && H >= 1 && capacity >= 1, "bad sizes");
    const long long gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    SPLAT_CHECK_ARG(gx * gy <= 0x7fffffffll / 2 && capacity <= 0x7fffffffll, "too many tiles or pairs");
    const int T = (int)(gx * gy);
    SPLAT_CHECK_ARG(n_active >= 0 && n_active <= T, "n_active must be in [0, T]");
    SPLAT_CHECK_ARG(active_tiles || n_active == 0 || n_active == T, "n_active must be T when active_tiles is NULL (every tile)");
    SPLAT_CHECK_ARG(uv && conic && opacity && feature && idx_sorted && tile_range && slot_sorted && target && tile_loss && pair_grad,
                    "null pointer");
    SPLAT_CHECK_ARG((uintptr_t)pair_grad % 16 == 0, "pair_grad must be 16-byte aligned");
    if (n_active == 0) return SPLAT_OK;
    FitArgs A;
    A.P = P;
    A.uv = (const float2 *)uv;
    A.conic = conic;
    A.opacity = opacity;
    A.feature = feature;
    A.idx_sorted = idx_sorted;
    A.tile_range = (const int2 *)tile_range;
    A.slot_sorted = slot_sorted;
    A.capacity = capacity;
    A.bg = bg;
    A.W = W;
    A.H = H;
    A.gx = (int)gx;
    A.T = T;
    A.target = target;
    A.pixel_weight = pixel_weight;
    A.active_tiles = active_tiles;
    A.tile_loss = tile_loss;
    A.pair_grad = (float4 *)pair_grad;
    A.out = out;
    A.ncontrib = ncontrib;
    A.inv_n = (float)(1.0 / (3.0 * (double)H * (double)W));
    SPLAT_LAUNCH("blend_fit_color", blend_fit_color_kernel, dim3((unsigned)n_active), dim3(256), 0, (hipStream_t)stream, A);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_tile_loss_sum(int T, const float *tile_loss, float *history, int64_t slot, splat_stream_t stream) {
    SPLAT_CHECK_ARG(T >= 1 && slot >= 0, "bad sizes");
    SPLAT_CHECK_ARG(tile_loss && history, "null pointer");
    SPLAT_LAUNCH("tile_loss_sum", tile_loss_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, T, tile_loss, history + slot);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}
