// Dense optical flow of the learned video (include/splat_hip_flow.h): the reference's get_pred_flows_gs
// (src/trainer_fragGS.py:777-821) composites uv(ids2) - uv(ids1) over the sorted lists of frame ids1 and colours the result
// with util.flow_to_image (src/util.py:421-536).  Here:
//   - the per-Gaussian flow attribute of a batch of frame pairs and its gradient (one launch each way),
//   - the Middlebury colouring on the device (maximum radius: partials + fold; colouring),
//   - the flow error sums against a reference flow with the gradient of the weighted-mean L1,
//   - (include/splat_hip_flow_occ.h) the attribute with the depth -- the same two kernels, templated on the channel count --
//     and the fused per-pixel occlusion / warp kernel, whose decisions follow from the bits of a float32 restatement.
// This file is compiled with -ffp-contract=off (Makefile): every product and sum below is rounded once, so that the two
// projections of a pair are the same instructions whatever the compiler inlines where (a pair of equal times gives +0.0)
// and the float32 steps of the colouring are the ones numpy takes.  The spline position alone carries one explicit
// fma, the one the compiler contracts dynamics.hip's expression into: it has to give the bits of positions_batch.
#include "common.h"
#include "dynamics_dev.h"
#include "pointwise_dev.h"
#include "../../include/splat_hip_flow_occ.h"

namespace {

constexpr int FLOW_BLOCK = 256;

// camera of pair f as the kernels take it (splat_camera_t without the fields they do not read)
struct FlowCam {
    const float *extr, *intr;
    long long extr_fs, intr_fs;
};

__device__ __forceinline__ void load_flow_cam(const FlowCam &fc, int f, Cam &c) {
    load_cam(fc.intr ? fc.intr + (size_t)f * fc.intr_fs : nullptr, fc.extr + (size_t)f * fc.extr_fs, c);
}

// get_position(t) of Gaussian n, all three axes: dynamic_eval_fwd_kernel's c3 + c2 d + c1 d^2 + c0 d^3 + base as the
// compiler builds it there and in dynamic_positions_fwd_kernel (read off their ISA: the first step is one fma, the products
// c1 (d d) and c0 ((d d) d) are rounded on their own -- the vectoriser pairs them into one packed multiply -- and added)
__device__ __forceinline__ void spline_position(const float *__restrict__ cubic, const CubicAddr &ca, size_t n, float d,
                                                const float base[3], float p[3]) {
    const float *c = cubic + ca.seg_off + n * ca.stride_n;
    const size_t row = ca.stride_k;
    const float d2 = d * d, d3 = d2 * d;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float c0 = c[j], c1 = c[row + j], c2 = c[2 * row + j], c3 = c[3 * row + j];
        float q = __builtin_fmaf(c2, d, c3);
        q = q + c1 * d2;
        q = q + c0 * d3;
        p[j] = q + base[j];
    }
}

template <bool PERSP>
__device__ __forceinline__ bool project_pt(const Cam &c, const float p[3], int W, int H, float nearest, float extent, float &u,
                                           float &v, float &d) {
    return PERSP ? project_persp_pt(c, p[0], p[1], p[2], W, H, nearest, extent, u, v, d)
                 : project_ortho_pt(c, p[0], p[1], p[2], W, H, nearest, extent, u, v, d);
}

// the attribute's row: NCH = 2 (u2 - u1, v2 - v1), NCH = 4 (..., z2 - z1, z2), one store of 8 or 16 bytes
template <int NCH> struct FlowRow;
template <> struct FlowRow<2> { using type = float2; };
template <> struct FlowRow<4> { using type = float4; };

// One lane per Gaussian walks its slice of the pairs (grid.y slices them as dynamic_positions_fwd_kernel slices its frames):
// base position read once, per pair the two 48-byte spline records, two projections, one 8-byte (NCH = 4: 16-byte) store.
template <bool PERSP, int NCH>
__global__ __launch_bounds__(FLOW_BLOCK) void flow_attribute_kernel(int F, int P, int I, int layout,
                                                                    const DynTab *__restrict__ tab1,
                                                                    const DynTab *__restrict__ tab2,
                                                                    const float *__restrict__ position,
                                                                    const float *__restrict__ cubic, FlowCam fc1, FlowCam fc2,
                                                                    int W, int H, float nearest, float extent, int zero_culled,
                                                                    typename FlowRow<NCH>::type *__restrict__ flow) {
    const size_t n = (size_t)blockIdx.x * FLOW_BLOCK + threadIdx.x;
    if (n >= (size_t)P) return;
    const float base[3] = {position[n * 3], position[n * 3 + 1], position[n * 3 + 2]};
    const int per = (F + gridDim.y - 1) / gridDim.y;
    const int f0 = blockIdx.y * per, f1 = imin_(F, f0 + per);
    for (int f = f0; f < f1; ++f) {
        float p1[3], p2[3], u1, v1, z1, u2, v2, z2;
        Cam c1, c2;
        spline_position(cubic, cubic_addr(layout, P, I, tab1[f].seg), n, tab1[f].d, base, p1);
        spline_position(cubic, cubic_addr(layout, P, I, tab2[f].seg), n, tab2[f].d, base, p2);
        load_flow_cam(fc1, f, c1);
        load_flow_cam(fc2, f, c2);
        const bool cull1 = project_pt<PERSP>(c1, p1, W, H, nearest, extent, u1, v1, z1);
        const bool cull2 = project_pt<PERSP>(c2, p2, W, H, nearest, extent, u2, v2, z2);
        if (cull1) u1 = v1 = z1 = 0.f;
        if (cull2) u2 = v2 = z2 = 0.f;
        const bool none = zero_culled && (cull1 || cull2);
        if constexpr (NCH == 2) {
            float2 o = make_float2(u2 - u1, v2 - v1);
            if (none) o = make_float2(0.f, 0.f);
            flow[(size_t)f * P + n] = o;
        } else {
            float4 o = make_float4(u2 - u1, v2 - v1, z2 - z1, z2);
            if (none) o = make_float4(0.f, 0.f, 0.f, 0.f);
            flow[(size_t)f * P + n] = o;
        }
    }
}

// Backward: the lane owns its Gaussian's rows of d_position and d_cubic (no atomics).  It walks the pairs in tab1's walk
// order (dynamic_positions_bwd_kernel's) and keeps, for each of the two times of a pair, the coefficient sums of the current
// segment in registers; a side's sums are added to memory when that side's walk leaves the segment.
template <bool PERSP, int NCH>
__global__ __launch_bounds__(FLOW_BLOCK) void flow_attribute_bwd_kernel(int F, int P, int I, int layout,
                                                                        const DynTab *__restrict__ tab1,
                                                                        const DynTab *__restrict__ tab2,
                                                                        const float *__restrict__ position,
                                                                        const float *__restrict__ cubic, FlowCam fc1,
                                                                        FlowCam fc2, int W, int H, float nearest, float extent,
                                                                        int zero_culled,
                                                                        const typename FlowRow<NCH>::type *__restrict__ g,
                                                                        float *__restrict__ d_position,
                                                                        float *__restrict__ d_cubic) {
    const size_t n = (size_t)blockIdx.x * FLOW_BLOCK + threadIdx.x;
    if (n >= (size_t)P) return;
    const float base[3] = {position[n * 3], position[n * 3 + 1], position[n * 3 + 2]};
    float acc[2][4][3], dpos[3] = {0.f, 0.f, 0.f};
    int cur[2] = {-1, -1};
    auto clear = [&](int s) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[s][k][j] = 0.f;
    };
    auto flush = [&](int s) {
        if (cur[s] < 0 || !d_cubic) return;
        const CubicAddr ca = cubic_addr(layout, P, I, cur[s]);
        float *c = d_cubic + ca.seg_off + n * ca.stride_n;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) c[k * ca.stride_k + j] += acc[s][k][j];
    };
    clear(0);
    clear(1);
    for (int i = 0; i < F; ++i) {
        const int o = __float_as_int(tab1[i].pad[0]);
        const int f = (o >= 1 && o <= F) ? o - 1 : i;
        const DynTab *tabs[2] = {tab1 + f, tab2 + f};
        float p[2][3], u, v, z;
        Cam c[2];
        bool cull[2];
        load_flow_cam(fc1, f, c[0]);
        load_flow_cam(fc2, f, c[1]);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            spline_position(cubic, cubic_addr(layout, P, I, tabs[s]->seg), n, tabs[s]->d, base, p[s]);
            cull[s] = project_pt<PERSP>(c[s], p[s], W, H, nearest, extent, u, v, z);
        }
        const auto gf = g[(size_t)f * P + n];
        const bool none = zero_culled && (cull[0] || cull[1]);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int seg = tabs[s]->seg;
            if (seg != cur[s]) {   // uniform: the table is the same for every lane
                flush(s);
                clear(s);
                cur[s] = seg;
            }
            if (none || cull[s]) continue;
            const float sg = s == 0 ? -1.f : 1.f;   // flow = uv2 - uv1
            float gd = 0.f;                          // NCH = 4: z2 - z1 and z2
            if constexpr (NCH == 4) gd = s == 0 ? -gf.z : gf.z + gf.w;
            float gp[3];
            if (PERSP) project_persp_grad_pt(c[s], p[s][0], p[s][1], p[s][2], sg * gf.x, sg * gf.y, gd, gp);
            else project_ortho_grad_pt(c[s], W, H, sg * gf.x, sg * gf.y, gd, gp);
            const float d = tabs[s]->d, d2 = d * d, d3 = d2 * d;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                dpos[j] += gp[j];
                acc[s][0][j] += gp[j] * d3; acc[s][1][j] += gp[j] * d2; acc[s][2][j] += gp[j] * d; acc[s][3][j] += gp[j];
            }
        }
    }
    flush(0);
    flush(1);
    if (d_position) {
#pragma unroll
        for (int j = 0; j < 3; ++j) d_position[n * 3 + j] += dpos[j];
    }
}

// the helpers' refusals carry the entry point's name
#define FLOW_CHECK(who, cond, msg)                 \
    do {                                           \
        if (!(cond)) {                             \
            splat_set_error("%s: %s", who, msg);   \
            return SPLAT_E_ARG;                    \
        }                                          \
    } while (0)

#define FLOW_CHECK_HIP(who, expr)                                                 \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            splat_set_error("%s: %s -> %s", who, #expr, hipGetErrorString(e_));   \
            return SPLAT_E_LAUNCH;                                                \
        }                                                                         \
    } while (0)

int flow_camera(const char *who, const splat_camera_t *cam, FlowCam &fc) {
    FLOW_CHECK(who, cam && cam->extr, "null camera (cam1 and its extr are required; cam2 may be NULL as a whole)");
    FLOW_CHECK(who, !cam->perspective || cam->intr, "the perspective camera needs intr");
    FLOW_CHECK(who, (cam->extr_frame_stride == 0 || cam->extr_frame_stride >= 12) &&
                        (cam->intr_frame_stride == 0 || cam->intr_frame_stride >= 4),
                    "negative camera stride, or rows that overlap (extr: 0 or >= 12 floats, intr: 0 or >= 4)");
    fc.extr = cam->extr;
    fc.intr = cam->perspective ? cam->intr : nullptr;
    fc.extr_fs = cam->extr_frame_stride;
    fc.intr_fs = cam->perspective ? cam->intr_frame_stride : 0;
    return SPLAT_OK;
}

// the checks both directions share; `persp` = the pinhole camera (both cameras of a pair are of one kind)
int flow_args(const char *who, int F, int P, int I, const void *tab1, const void *tab2, const float *position, const float *cubic, int cubic_layout,
              const splat_camera_t *cam1, const splat_camera_t *cam2, int W, int H, FlowCam &fc1, FlowCam &fc2, bool &persp) {
    FLOW_CHECK(who, F >= 0 && F <= 65535 && P >= 0 && I >= 1 && W > 0 && H > 0, "bad sizes");
    FLOW_CHECK(who, cubic_layout == SPLAT_CUBIC_GAUSSIAN_MAJOR || cubic_layout == SPLAT_CUBIC_SEGMENT_MAJOR, "unknown cubic_layout");
    if (int rc = flow_camera(who, cam1, fc1)) return rc;
    fc2 = fc1;
    if (cam2) {
        if (int rc = flow_camera(who, cam2, fc2)) return rc;
        FLOW_CHECK(who, !cam1->perspective == !cam2->perspective, "cam1 and cam2 must both be orthographic or both pinhole");
    }
    persp = cam1->perspective != 0;
    if (F == 0 || P == 0) return SPLAT_OK;
    FLOW_CHECK(who, tab1 && tab2 && position && cubic, "null input pointer");
    return SPLAT_OK;
}

// ---------------------------------------------------------------------------------------------------------------- colours
// Scharstein's wheel (make_colorwheel): 55 rows r g b, integers 0 .. 255 (floor(255 k / n) ramps)
struct Wheel {
    unsigned char c[55][3];
};
constexpr Wheel make_wheel() {
    Wheel w{};
    const int RY = 15, YG = 6, GC = 4, CB = 11, BM = 13, MR = 6;
    int col = 0;
    for (int k = 0; k < RY; ++k) { w.c[col + k][0] = 255; w.c[col + k][1] = (unsigned char)(255 * k / RY); }
    col += RY;
    for (int k = 0; k < YG; ++k) { w.c[col + k][0] = (unsigned char)(255 - 255 * k / YG); w.c[col + k][1] = 255; }
    col += YG;
    for (int k = 0; k < GC; ++k) { w.c[col + k][1] = 255; w.c[col + k][2] = (unsigned char)(255 * k / GC); }
    col += GC;
    for (int k = 0; k < CB; ++k) { w.c[col + k][1] = (unsigned char)(255 - 255 * k / CB); w.c[col + k][2] = 255; }
    col += CB;
    for (int k = 0; k < BM; ++k) { w.c[col + k][2] = 255; w.c[col + k][0] = (unsigned char)(255 * k / BM); }
    col += BM;
    for (int k = 0; k < MR; ++k) { w.c[col + k][2] = (unsigned char)(255 - 255 * k / MR); w.c[col + k][0] = 255; }
    return w;
}
__constant__ Wheel WHEEL = make_wheel();

constexpr int PIX_ITEMS = 8;                           // pixels per thread of a partial
constexpr int PIX_PER_BLOCK = FLOW_BLOCK * PIX_ITEMS;  // 2048 pixels per workgroup

inline int pix_blocks(int H, int W) { return (int)(((size_t)H * W + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK); }

__device__ __forceinline__ float clip_component(float x, float clip) {
    // np.clip(x, 0, clip): minimum(maximum(x, 0), clip); a NaN stays a NaN
    if (clip > 0.f && x == x) x = fminf(fmaxf(x, 0.f), clip);
    return x;
}

// pass 1: partial[f][b] = max of sqrt(u*u + v*v) over the block's pixels with finite u and v (0 when it has none)
__global__ __launch_bounds__(FLOW_BLOCK) void flow_radmax_partial_kernel(int HW, const float *__restrict__ flow, float clip,
                                                                        float *__restrict__ partial) {
    const int f = blockIdx.y, nb = gridDim.x;
    const float *u = flow + (size_t)f * 2 * HW, *v = u + HW;
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < PIX_ITEMS; ++k) {
        const int i = blockIdx.x * PIX_PER_BLOCK + k * FLOW_BLOCK + threadIdx.x;
        if (i < HW) {
            const float a = clip_component(u[i], clip), b = clip_component(v[i], clip);
            const float r = sqrtf(a * a + b * b);
            if (isfinite(a) && isfinite(b) && isfinite(r)) m = fmaxf(m, r);
        }
    }
    __shared__ float sm[FLOW_BLOCK];
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = FLOW_BLOCK / 2; s > 0; s >>= 1) {   // fixed tree
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)f * nb + blockIdx.x] = sm[0];
}

// fold: rad_max[f] = max over the partials of map f (whole_clip: of all maps), ascending order, one workgroup
__global__ __launch_bounds__(64) void flow_radmax_fold_kernel(int F, int nb, int whole_clip, const float *__restrict__ partial,
                                                             float *__restrict__ rad_max) {
    const int f = threadIdx.x + blockIdx.x * 64;
    if (f >= F) return;
    const int lo = whole_clip ? 0 : f * nb, hi = whole_clip ? F * nb : (f + 1) * nb;
    float m = 0.f;
    for (int i = lo; i < hi; ++i) m = fmaxf(m, partial[i]);
    rad_max[f] = m;
}

// pass 2: flow_uv_to_colors.  float32: u / (rad_max + 1e-5), rad, arctan2(-v, -u) / pi, fk = (a + 1) / 2 * 54, f = fk - k0;
// float64: col = (1 - f) c0 + f c1, 1 - rad (1 - col) | col * 0.75, floor(255 col)
__global__ __launch_bounds__(FLOW_BLOCK) void flow_colour_kernel(int HW, const float *__restrict__ flow, float clip,
                                                                const float *__restrict__ rad_max, float rad_given, int bgr,
                                                                unsigned char *__restrict__ out) {
    const int f = blockIdx.y;
    const int i = blockIdx.x * FLOW_BLOCK + threadIdx.x;
    if (i >= HW) return;
    const float *up = flow + (size_t)f * 2 * HW, *vp = up + HW;
    const float rm = rad_max ? rad_max[f] : rad_given;
    const float den = rm + 1e-5f;
    const float u0 = clip_component(up[i], clip), v0 = clip_component(vp[i], clip);
    unsigned char *px = out + ((size_t)f * HW + i) * 3;
    if (!(isfinite(u0) && isfinite(v0))) {
        px[0] = px[1] = px[2] = 0;
        return;
    }
    const float u = u0 / den, v = v0 / den;
    const float rad = sqrtf(u * u + v * v);
    const float a = atan2f(-v, -u) / 3.14159265358979323846f;
    const float fk = (a + 1.f) / 2.f * 54.f;
    int k0 = (int)floorf(fk);
    k0 = imin_(imax_(k0, 0), 54);
    const int k1 = k0 == 54 ? 0 : k0 + 1;
    const double fr = (double)(fk - (float)k0);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double c0 = (double)WHEEL.c[k0][ch] / 255.0, c1 = (double)WHEEL.c[k1][ch] / 255.0;
        double col = (1.0 - fr) * c0 + fr * c1;
        if (rad <= 1.f) col = 1.0 - (double)rad * (1.0 - col);
        else col = col * 0.75;
        const double lv = floor(255.0 * col);
        px[bgr ? 2 - ch : ch] = (unsigned char)(lv < 0.0 ? 0.0 : (lv > 255.0 ? 255.0 : lv));
    }
}

// ---------------------------------------------------------------------------------------------------------------- error
// sum over the workgroup in a fixed tree: wave sums by DPP, then the four wave totals in ascending order
__device__ __forceinline__ float block_sum(float v, float *sm) {
    v = wave_sum_to_lane63(v);
    if ((threadIdx.x & 63) == 63) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    __syncthreads();
    return t;
}

// partial[(f * nb + b) * 3 + {0,1,2}] = float32 sums over the block's 2048 pixels of w (|du| + |dv|), w sqrt(du^2 + dv^2), w
__global__ __launch_bounds__(FLOW_BLOCK) void flow_error_partial_kernel(int HW, const float *__restrict__ pred,
                                                                       const float *__restrict__ gt,
                                                                       const float *__restrict__ weight,
                                                                       float *__restrict__ partial) {
    const int f = blockIdx.y, nb = gridDim.x;
    const size_t o = (size_t)f * 2 * HW;
    float s1 = 0.f, s2 = 0.f, sw = 0.f;
#pragma unroll
    for (int k = 0; k < PIX_ITEMS; ++k) {
        const int i = blockIdx.x * PIX_PER_BLOCK + k * FLOW_BLOCK + threadIdx.x;
        if (i < HW) {
            const float w = weight ? weight[(size_t)f * HW + i] : 1.f;
            const float du = pred[o + i] - gt[o + i], dv = pred[o + HW + i] - gt[o + HW + i];
            s1 += w * (fabsf(du) + fabsf(dv));
            s2 += w * sqrtf(du * du + dv * dv);
            sw += w;
        }
    }
    __shared__ float sm[4];
    s1 = block_sum(s1, sm);
    s2 = block_sum(s2, sm);
    sw = block_sum(sw, sm);
    if (threadIdx.x == 0) {
        float *p = partial + ((size_t)f * nb + blockIdx.x) * 3;
        p[0] = s1; p[1] = s2; p[2] = sw;
    }
}

// sums[f][c] = the partials of map f folded in float64, ascending block order; thread = (map, sum)
__global__ __launch_bounds__(64) void flow_error_fold_kernel(int F, int nb, const float *__restrict__ partial,
                                                            double *__restrict__ sums) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= F * 3) return;
    const int f = t / 3, c = t - 3 * f;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += (double)partial[((size_t)f * nb + b) * 3 + c];
    sums[t] = s;
}

__device__ __forceinline__ float sign_f(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// grad = (scale / max(sum_f w, 1e-30), rounded to float32 once) * w * sign(d)
__global__ __launch_bounds__(FLOW_BLOCK) void flow_error_grad_kernel(int HW, const float *__restrict__ pred,
                                                                    const float *__restrict__ gt,
                                                                    const float *__restrict__ weight, float scale,
                                                                    const double *__restrict__ sums, float *__restrict__ grad) {
    const int f = blockIdx.y;
    const int i = blockIdx.x * FLOW_BLOCK + threadIdx.x;
    if (i >= HW) return;
    const double sw = sums[f * 3 + 2];
    const float k = (float)((double)scale / (sw > 1e-30 ? sw : 1e-30));
    const float w = weight ? weight[(size_t)f * HW + i] : 1.f;
    const size_t o = (size_t)f * 2 * HW;
    const float kw = k * w;
    grad[o + i] = kw * sign_f(pred[o + i] - gt[o + i]);
    grad[o + HW + i] = kw * sign_f(pred[o + HW + i] - gt[o + HW + i]);
}

}  // namespace

extern "C" int splat_flow_abi_version(void) { return SPLAT_FLOW_ABI_VERSION; }

namespace {

// both channel counts: the checks, the grid and the launch of the forward (`who`: the entry point's name)
template <int NCH>
int flow_attribute_launch(const char *who, int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                          const float *cubic, int cubic_layout, const splat_camera_t *cam1, const splat_camera_t *cam2, int W,
                          int H, float nearest, float extent, int zero_culled, float *flow, void *stream) {
    using Row = typename FlowRow<NCH>::type;
    FlowCam fc1, fc2;
    bool persp = false;
    if (int rc = flow_args(who, F, P, I, tab1, tab2, position, cubic, cubic_layout, cam1, cam2, W, H, fc1, fc2, persp)) return rc;
    if (F == 0 || P == 0) return SPLAT_OK;
    FLOW_CHECK(who, flow != nullptr && ((uintptr_t)flow & (sizeof(Row) - 1)) == 0,
               NCH == 2 ? "null / misaligned output (flow: 8-byte aligned)" : "null / misaligned output (out: 16-byte aligned)");
    const unsigned blocks = (unsigned)(((size_t)P + FLOW_BLOCK - 1) / FLOW_BLOCK);
    unsigned slices = 1;   // enough workgroups to fill the chip: slice the pairs when the Gaussians alone do not
    while (blocks * slices < 2048u && slices < (unsigned)F) slices *= 2;
    if (slices > (unsigned)F) slices = (unsigned)F;
    const dim3 grid(blocks, slices);
    hipStream_t s = (hipStream_t)stream;
    if (persp)
        SPLAT_LAUNCH("flow_attribute", (flow_attribute_kernel<true, NCH>), grid, dim3(FLOW_BLOCK), 0, s, F, P, I, cubic_layout,
                     (const DynTab *)tab1, (const DynTab *)tab2, position, cubic, fc1, fc2, W, H, nearest, extent, zero_culled,
                     (Row *)flow);
    else
        SPLAT_LAUNCH("flow_attribute", (flow_attribute_kernel<false, NCH>), grid, dim3(FLOW_BLOCK), 0, s, F, P, I, cubic_layout,
                     (const DynTab *)tab1, (const DynTab *)tab2, position, cubic, fc1, fc2, W, H, nearest, extent, zero_culled,
                     (Row *)flow);
    FLOW_CHECK_HIP(who, hipGetLastError());
    return SPLAT_OK;
}

template <int NCH>
int flow_attribute_bwd_launch(const char *who, int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                              const float *cubic, int cubic_layout, const splat_camera_t *cam1, const splat_camera_t *cam2,
                              int W, int H, float nearest, float extent, int zero_culled, const float *g, int accumulate,
                              float *d_position, float *d_cubic, void *stream) {
    using Row = typename FlowRow<NCH>::type;
    FlowCam fc1, fc2;
    bool persp = false;
    if (int rc = flow_args(who, F, P, I, tab1, tab2, position, cubic, cubic_layout, cam1, cam2, W, H, fc1, fc2, persp)) return rc;
    if (P == 0 || (!d_position && !d_cubic)) return SPLAT_OK;
    if (F > 0)   // in front of any HIP call
        FLOW_CHECK(who, g != nullptr && ((uintptr_t)g & (sizeof(Row) - 1)) == 0,
                   NCH == 2 ? "null / misaligned gradient (g: 8-byte aligned)" : "null / misaligned gradient (g: 16-byte aligned)");
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) {
        if (d_position) FLOW_CHECK_HIP(who, hipMemsetAsync(d_position, 0, (size_t)P * 3 * sizeof(float), s));
        if (d_cubic) FLOW_CHECK_HIP(who, hipMemsetAsync(d_cubic, 0, (size_t)P * 12 * (size_t)I * sizeof(float), s));
    }
    if (F == 0) return SPLAT_OK;
    const dim3 grid((unsigned)(((size_t)P + FLOW_BLOCK - 1) / FLOW_BLOCK));
    if (persp)
        SPLAT_LAUNCH("flow_attribute_bwd", (flow_attribute_bwd_kernel<true, NCH>), grid, dim3(FLOW_BLOCK), 0, s, F, P, I,
                     cubic_layout, (const DynTab *)tab1, (const DynTab *)tab2, position, cubic, fc1, fc2, W, H, nearest, extent,
                     zero_culled, (const Row *)g, d_position, d_cubic);
    else
        SPLAT_LAUNCH("flow_attribute_bwd", (flow_attribute_bwd_kernel<false, NCH>), grid, dim3(FLOW_BLOCK), 0, s, F, P, I,
                     cubic_layout, (const DynTab *)tab1, (const DynTab *)tab2, position, cubic, fc1, fc2, W, H, nearest, extent,
                     zero_culled, (const Row *)g, d_position, d_cubic);
    FLOW_CHECK_HIP(who, hipGetLastError());
    return SPLAT_OK;
}

}  // namespace

extern "C" int splat_flow_attribute_batch(int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                                          const float *cubic, int cubic_layout, const splat_camera_t *cam1,
                                          const splat_camera_t *cam2, int W, int H, float nearest, float extent, int zero_culled,
                                          float *flow, void *stream) {
    return flow_attribute_launch<2>(__func__, F, P, I, tab1, tab2, position, cubic, cubic_layout, cam1, cam2, W, H, nearest, extent,
                                    zero_culled, flow, stream);
}

extern "C" int splat_flow_attribute_batch_backward(int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                                                   const float *cubic, int cubic_layout, const splat_camera_t *cam1,
                                                   const splat_camera_t *cam2, int W, int H, float nearest, float extent,
                                                   int zero_culled, const float *g, int accumulate, float *d_position,
                                                   float *d_cubic, void *stream) {
    return flow_attribute_bwd_launch<2>(__func__, F, P, I, tab1, tab2, position, cubic, cubic_layout, cam1, cam2, W, H, nearest,
                                        extent, zero_culled, g, accumulate, d_position, d_cubic, stream);
}

extern "C" size_t splat_flow_scratch_bytes(int F, int H, int W) {
    if (F < 1 || H < 1 || W < 1) return 0;
    return (size_t)F * (size_t)pix_blocks(H, W) * 3 * sizeof(float);
}

static int flow_maps(int F, int H, int W, const char *&why) {
    why = nullptr;
    if (!(F >= 0 && F <= 65535 && H > 0 && W > 0 && (long long)H * W <= 0x3fffffffLL)) why = "bad sizes (F 0 .. 65535, H * W <= 2^30 - 1)";
    return why ? SPLAT_E_ARG : SPLAT_OK;
}

extern "C" int splat_flow_to_image(int F, int H, int W, const float *flow, float clip_flow, int scale_mode, float rad_max_in,
                                   float *rad_max_out, uint8_t *out, int bgr, void *scratch, size_t scratch_bytes,
                                   void *stream) {
    const char *why;
    flow_maps(F, H, W, why);
    SPLAT_CHECK_ARG(!why, why);
    SPLAT_CHECK_ARG(scale_mode == SPLAT_FLOW_SCALE_PER_FRAME || scale_mode == SPLAT_FLOW_SCALE_WHOLE_CLIP ||
                        scale_mode == SPLAT_FLOW_SCALE_GIVEN, "unknown scale_mode");
    SPLAT_CHECK_ARG(clip_flow == clip_flow, "clip_flow is NaN");
    const bool given = scale_mode == SPLAT_FLOW_SCALE_GIVEN;
    SPLAT_CHECK_ARG(!given || (rad_max_in >= 0.f && rad_max_in <= 3.4028234663852886e38f), "rad_max_in must be finite and >= 0");
    if (F == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(flow && out, "null pointer");
    const int HW = H * W, nb = pix_blocks(H, W);
    hipStream_t s = (hipStream_t)stream;
    float *partial = (float *)scratch, *rad_max = nullptr;
    if (!given) {
        // partials [F * nb], then the F maxima (inside the 3 floats per block the scratch holds)
        SPLAT_CHECK_ARG(scratch && ((uintptr_t)scratch & 3) == 0 && scratch_bytes >= splat_flow_scratch_bytes(F, H, W),
                        "scratch missing or too small (splat_flow_scratch_bytes)");
        rad_max = partial + (size_t)F * nb;
        SPLAT_LAUNCH("flow_radmax_partial", flow_radmax_partial_kernel, dim3(nb, F), dim3(FLOW_BLOCK), 0, s, HW, flow, clip_flow,
                     partial);
        SPLAT_LAUNCH("flow_radmax_fold", flow_radmax_fold_kernel, dim3((F + 63) / 64), dim3(64), 0, s, F, nb,
                     scale_mode == SPLAT_FLOW_SCALE_WHOLE_CLIP ? 1 : 0, partial, rad_max);
    }
    SPLAT_LAUNCH("flow_colour", flow_colour_kernel, dim3((HW + FLOW_BLOCK - 1) / FLOW_BLOCK, F), dim3(FLOW_BLOCK), 0, s, HW, flow,
                 clip_flow, rad_max, rad_max_in, bgr, out);
    if (rad_max_out) {
        if (given) {
            for (int f = 0; f < F; ++f)   // F small host writes of one float (a clip's frames): stream-ordered
                SPLAT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(rad_max_out + f), __builtin_bit_cast(int, rad_max_in), 1, s));
        } else {
            SPLAT_CHECK_HIP(hipMemcpyAsync(rad_max_out, rad_max, (size_t)F * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_flow_error(int F, int H, int W, const float *pred, const float *gt, const float *weight, float scale,
                                double *sums, float *grad, void *scratch, size_t scratch_bytes, void *stream) {
    const char *why;
    flow_maps(F, H, W, why);
    SPLAT_CHECK_ARG(!why, why);
    SPLAT_CHECK_ARG(scale == scale && scale - scale == 0.f, "scale must be finite");
    if (F == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(pred && gt && sums, "null pointer");
    SPLAT_CHECK_ARG(((uintptr_t)sums & 7) == 0, "misaligned sums (double)");
    SPLAT_CHECK_ARG(scratch && ((uintptr_t)scratch & 3) == 0 && scratch_bytes >= splat_flow_scratch_bytes(F, H, W),
                    "scratch missing or too small (splat_flow_scratch_bytes)");
    const int HW = H * W, nb = pix_blocks(H, W);
    hipStream_t s = (hipStream_t)stream;
    float *partial = (float *)scratch;
    SPLAT_LAUNCH("flow_error_partial", flow_error_partial_kernel, dim3(nb, F), dim3(FLOW_BLOCK), 0, s, HW, pred, gt, weight,
                 partial);
    SPLAT_LAUNCH("flow_error_fold", flow_error_fold_kernel, dim3((F * 3 + 63) / 64), dim3(64), 0, s, F, nb, partial, sums);
    if (grad)
        SPLAT_LAUNCH("flow_error_grad", flow_error_grad_kernel, dim3((HW + FLOW_BLOCK - 1) / FLOW_BLOCK, F), dim3(FLOW_BLOCK), 0, s,
                     HW, pred, gt, weight, scale, sums, grad);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

// ---------------------------------------------------------------------------------------------------------------- occlusion
// include/splat_hip_flow_occ.h.  The attribute with the depth is the NCH = 4 instantiation of the kernels above.
extern "C" int splat_flow_occ_abi_version(void) { return SPLAT_FLOW_OCC_ABI_VERSION; }

extern "C" int splat_flow_attribute_depth_batch(int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                                                const float *cubic, int cubic_layout, const splat_camera_t *cam1,
                                                const splat_camera_t *cam2, int W, int H, float nearest, float extent,
                                                int zero_culled, float *out, void *stream) {
    return flow_attribute_launch<4>(__func__, F, P, I, tab1, tab2, position, cubic, cubic_layout, cam1, cam2, W, H, nearest, extent,
                                    zero_culled, out, stream);
}

extern "C" int splat_flow_attribute_depth_batch_backward(int F, int P, int I, const void *tab1, const void *tab2,
                                                         const float *position, const float *cubic, int cubic_layout,
                                                         const splat_camera_t *cam1, const splat_camera_t *cam2, int W, int H,
                                                         float nearest, float extent, int zero_culled, const float *g,
                                                         int accumulate, float *d_position, float *d_cubic, void *stream) {
    return flow_attribute_bwd_launch<4>(__func__, F, P, I, tab1, tab2, position, cubic, cubic_layout, cam1, cam2, W, H, nearest,
                                        extent, zero_culled, g, accumulate, d_position, d_cubic, stream);
}

namespace {

struct OccArgs {
    const float *flow, *track_depth, *surface, *coverage, *flow_back, *src;
    float bg_depth, depth_margin, min_coverage, fb_alpha, fb_beta;
    unsigned char *mask;
    float *depth_gap, *fb_sq, *warped;
    int *partial;   // [F][blocks][4] or NULL
};

// V consecutive floats / bytes of a plane: one 16-byte (4-byte) access when V = 4 -- the host picks V = 4 only when every
// plane of every map starts on a 16-byte boundary (H * W a multiple of 4, aligned base pointers)
template <int V>
__device__ __forceinline__ void load_run(const float *__restrict__ p, float o[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
        o[0] = p[0];
    }
}
template <int V>
__device__ __forceinline__ void store_run(float *__restrict__ p, const float o[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(o[0], o[1], o[2], o[3]);
    else p[0] = o[0];
}

// the four corners and the two weights of q in an H x W plane; q is inside [0, W - 1] x [0, H - 1]
struct Corners {
    int o00, o01, o10, o11;
    float fx, fy, gx, gy;   // gx = 1 - fx
};
__device__ __forceinline__ Corners corners(float qx, float qy, int W, int H) {
    const float x0f = floorf(qx), y0f = floorf(qy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int x1 = imin_(x0 + 1, W - 1), y1 = imin_(y0 + 1, H - 1);
    Corners c;
    c.o00 = y0 * W + x0; c.o01 = y0 * W + x1; c.o10 = y1 * W + x0; c.o11 = y1 * W + x1;
    c.fx = qx - x0f; c.fy = qy - y0f;
    c.gx = 1.f - c.fx; c.gy = 1.f - c.fy;
    return c;
}
__device__ __forceinline__ float bilinear(const float *__restrict__ plane, const Corners &c) {
    const float v00 = plane[c.o00], v01 = plane[c.o01], v10 = plane[c.o10], v11 = plane[c.o11];
    return ((v00 * c.gx) + (v01 * c.fx)) * c.gy + ((v10 * c.gx) + (v11 * c.fx)) * c.fy;
}

// A thread takes PIX_ITEMS / V runs of V consecutive pixels (flow.hip's pixels-per-thread idiom; a wave's runs are contiguous):
// the pixel's own planes (flow, track depth, coverage) are read once in runs, the outputs stored in runs; the four-corner
// gathers of neighbouring pixels overlap (a flow field is smooth) and come from the cache.
template <int V>
__global__ __launch_bounds__(FLOW_BLOCK) void flow_occlusion_kernel(int H, int W, int C, OccArgs a) {
    const int f = blockIdx.y, HW = H * W;
    const size_t m = (size_t)f * HW;                  // offset of map f in a one-plane tensor
    const float *fu = a.flow + 2 * m, *fv = fu + HW;
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    int cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PIX_ITEMS / V; ++k) {
        const int i0 = blockIdx.x * PIX_PER_BLOCK + (k * FLOW_BLOCK + (int)threadIdx.x) * V;
        if (i0 >= HW) continue;                       // V = 4: HW is a multiple of 4, a run is inside or outside as a whole
        float u[V], v[V], td[V], cov[V], gap[V], fb[V];
        unsigned char bits[V];
        Corners cs[V];
        bool in[V];
        load_run<V>(fu + i0, u);
        load_run<V>(fv + i0, v);
        if (a.track_depth) load_run<V>(a.track_depth + m + i0, td);
        if (a.coverage) load_run<V>(a.coverage + m + i0, cov);
        const int y = i0 / W;
        int x = i0 - y * W, yy = y;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (x >= W) { x -= W; ++yy; }             // a run may cross the end of a row
            const float qx = (float)x + u[j], qy = (float)yy + v[j];
            const bool inside = qx >= 0.f && qx <= wmax && qy >= 0.f && qy <= hmax;      // false for a NaN
            unsigned b = inside ? 0u : (unsigned)SPLAT_FLOW_OCC_OUTSIDE;
            if (a.coverage && !(cov[j] >= a.min_coverage)) b |= SPLAT_FLOW_OCC_UNCOVERED;
            const bool decide = b == 0u;
            gap[j] = 0.f;
            fb[j] = 0.f;
            if (inside) {
                const Corners c = corners(qx, qy, W, H);
                if (a.surface) {
                    const float s = bilinear(a.surface + m, c);
                    float t = td[j];
                    if (a.coverage) t = t + (1.f - cov[j]) * a.bg_depth;
                    gap[j] = t - s;
                    if (decide && gap[j] > a.depth_margin) b |= SPLAT_FLOW_OCC_IN_FRONT;
                }
                if (a.flow_back) {
                    const float bu = bilinear(a.flow_back + 2 * m, c), bv = bilinear(a.flow_back + 2 * m + HW, c);
                    const float ru = u[j] + bu, rv = v[j] + bv;
                    fb[j] = ru * ru + rv * rv;
                    const float lim = a.fb_alpha * ((u[j] * u[j] + v[j] * v[j]) + (bu * bu + bv * bv)) + a.fb_beta;
                    if (decide && fb[j] > lim) b |= SPLAT_FLOW_OCC_INCONSISTENT;
                }
                cs[j] = c;
            }
            in[j] = inside;
            bits[j] = (unsigned char)b;
#pragma unroll
            for (int t = 0; t < 4; ++t) cnt[t] += (int)((b >> t) & 1u);
            ++x;
        }
        if constexpr (V == 4) *reinterpret_cast<uchar4 *>(a.mask + m + i0) = make_uchar4(bits[0], bits[1], bits[2], bits[3]);
        else a.mask[m + i0] = bits[0];
        if (a.depth_gap) store_run<V>(a.depth_gap + m + i0, gap);
        if (a.fb_sq) store_run<V>(a.fb_sq + m + i0, fb);
        if (a.warped) {
            for (int ch = 0; ch < C; ++ch) {
                const size_t o = ((size_t)f * C + ch) * HW;
                float w[V];
#pragma unroll
                for (int j = 0; j < V; ++j) w[j] = in[j] ? bilinear(a.src + o, cs[j]) : 0.f;
                store_run<V>(a.warped + o + i0, w);
            }
        }
    }
    if (a.partial) {   // integer sums: any order gives the same counts
        __shared__ int sm[4];
        if (threadIdx.x < 4) sm[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (cnt[t]) atomicAdd(&sm[t], cnt[t]);
        __syncthreads();
        if (threadIdx.x < 4) a.partial[((size_t)f * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = sm[threadIdx.x];
    }
}

// counts[f][bit] = the partials of map f; thread = (map, bit)
__global__ __launch_bounds__(64) void flow_occlusion_fold_kernel(int F, int nb, const int *__restrict__ partial,
                                                                int *__restrict__ counts) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= F * 4) return;
    const int f = t >> 2, c = t & 3;
    int s = 0;
    for (int b = 0; b < nb; ++b) s += partial[((size_t)f * nb + b) * 4 + c];
    counts[t] = s;
}

}  // namespace

extern "C" size_t splat_flow_occlusion_scratch_bytes(int F, int H, int W) {
    if (F < 1 || H < 1 || W < 1) return 0;
    return (size_t)F * (size_t)pix_blocks(H, W) * 4 * sizeof(int);
}

extern "C" int splat_flow_occlusion(int F, int H, int W, int C, const float *flow, const float *track_depth, const float *surface,
                                    const float *coverage, const float *flow_back, const float *src, float bg_depth,
                                    float depth_margin, float min_coverage, float fb_alpha, float fb_beta, uint8_t *mask,
                                    float *depth_gap, float *fb_sq, float *warped, int *counts, void *scratch,
                                    size_t scratch_bytes, void *stream) {
    const char *why;
    flow_maps(F, H, W, why);
    SPLAT_CHECK_ARG(!why, why);
    SPLAT_CHECK_ARG(!track_depth == !surface, "track_depth and surface are given both or neither");
    SPLAT_CHECK_ARG(src ? (C >= 1 && C <= 8) : C == 0, "src needs 1 <= C <= 8 planes (C == 0 without src)");
    SPLAT_CHECK_ARG(!depth_gap || surface, "depth_gap needs track_depth and surface");
    SPLAT_CHECK_ARG(!fb_sq || flow_back, "fb_sq needs flow_back");
    SPLAT_CHECK_ARG(!warped == !src, "warped and src are given both or neither");
    SPLAT_CHECK_ARG(bg_depth == bg_depth && depth_margin == depth_margin && min_coverage == min_coverage && fb_alpha == fb_alpha &&
                        fb_beta == fb_beta, "a NaN parameter");
    if (F == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(flow && mask, "null pointer (flow and mask are required)");
    SPLAT_CHECK_ARG((((uintptr_t)flow | (uintptr_t)track_depth | (uintptr_t)surface | (uintptr_t)coverage | (uintptr_t)flow_back |
                      (uintptr_t)src | (uintptr_t)depth_gap | (uintptr_t)fb_sq | (uintptr_t)warped | (uintptr_t)counts) & 3) == 0,
                    "misaligned pointer (float / int: 4-byte aligned)");
    const int HW = H * W, nb = pix_blocks(H, W);
    SPLAT_CHECK_ARG(!counts || (scratch && ((uintptr_t)scratch & 3) == 0 &&
                                scratch_bytes >= splat_flow_occlusion_scratch_bytes(F, H, W)),
                    "scratch missing or too small (splat_flow_occlusion_scratch_bytes)");
    OccArgs a{flow, track_depth, surface, coverage, flow_back, src, bg_depth, depth_margin, min_coverage, fb_alpha, fb_beta,
              mask, depth_gap, fb_sq, warped, counts ? (int *)scratch : nullptr};
    // runs of four pixels when every plane of every map starts on a 16-byte boundary (the mask: 4 bytes)
    const bool wide = (HW & 3) == 0 && (((uintptr_t)flow | (uintptr_t)track_depth | (uintptr_t)coverage | (uintptr_t)depth_gap |
                                         (uintptr_t)fb_sq | (uintptr_t)warped) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (wide) SPLAT_LAUNCH("flow_occlusion", flow_occlusion_kernel<4>, dim3(nb, F), dim3(FLOW_BLOCK), 0, s, H, W, C, a);
    else SPLAT_LAUNCH("flow_occlusion", flow_occlusion_kernel<1>, dim3(nb, F), dim3(FLOW_BLOCK), 0, s, H, W, C, a);
    if (counts)
        SPLAT_LAUNCH("flow_occlusion_fold", flow_occlusion_fold_kernel, dim3((F * 4 + 63) / 64), dim3(64), 0, s, F, nb,
                     (const int *)scratch, counts);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}
