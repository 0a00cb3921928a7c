// Seeding the dynamic Gaussians from a clip's data: what the reference does on the CPU before its first training step.
//
//   K1 median_kernel<K>   K x K median filter with reflect padding (src/video3Dflow/utils.py:198-210 with same=True, the depth
//                         maps of video_3d_flow.py:131-137): one workgroup per 32 x 8 output tile, the padded tile staged in LDS
//                         once as order-preserving integer keys; every thread holds its K*K window in registers and finds the key
//                         of rank (K*K-1)/2 by a 32-step bisection over the key bits (a count of "key < candidate" per step).
//                         A selection, no arithmetic: the output is one of the input values, bit for bit.
//   K2 lift_kernel        a wave per track, a lane per frame: TAPIR visibility / confidence, bilinear depth (border padding) and
//                         mask (zero padding) samples, the orthographic 3-D point, per-track visible / confident counts (integer
//                         wave reduction), and the query-frame colour (utils.py:69-174).  The bilinear arithmetic is the plain
//                         float32 formula of torch's grid_sample(align_corners=True) with every product and sum rounded once:
//                         the in-mask decision is a float equality, so this file is compiled with contraction off.
//   K3 spline_kernel      a thread per (Gaussian, coordinate): not-a-knot cubic spline through the knot frames
//                         (src/dynamic_gaussian_with_base_point_cloud.py:66-78, scipy.interpolate.CubicSpline).  The tridiagonal
//                         matrix of the knot slopes depends on the knots only: the host factors it in float64 (Thomas), the kernel
//                         does the two substitution sweeps in float64 (the swept right-hand side lives in LDS), forms the four
//                         coefficients in float64 and stores float32 -- a float64 solve rounded once, as the reference's.
// No float atomics anywhere: every entry point runs under splat_set_deterministic(1).
#include "common.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------------- median
constexpr int MED_TX = 32, MED_TY = 8, MED_THREADS = MED_TX * MED_TY;

__device__ __forceinline__ unsigned med_key(float f) {  // order-preserving map float -> uint
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float med_unkey(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ int med_reflect(int p, int n) {  // reflect padding (no edge repeat); n > K/2
    p = p < 0 ? -p : p;
    p = p >= n ? 2 * (n - 1) - p : p;
    return imin_(imax_(p, 0), n - 1);  // (columns / rows past the image in an edge tile: any valid address, never stored)
}

template <int K>
__global__ void __launch_bounds__(MED_THREADS)
median_kernel(int H, int W, int tiles_x, int tiles_y, const float *__restrict__ x, float *__restrict__ out) {
    constexpr int R = K / 2, PW = MED_TX + 2 * R, PH = MED_TY + 2 * R, KK = K * K, RANK = (KK - 1) / 2;
    __shared__ unsigned tile[PH * PW];
    const int b = blockIdx.x;
    const int tx = b % tiles_x, ty = (b / tiles_x) % tiles_y, plane = b / (tiles_x * tiles_y);
    const size_t base = (size_t)plane * (size_t)H * (size_t)W;
    const int ox = tx * MED_TX, oy = ty * MED_TY;
    for (int e = threadIdx.x; e < PH * PW; e += MED_THREADS) {
        const int ly = e / PW, lx = e - ly * PW;
        const int gy = med_reflect(oy + ly - R, H), gx = med_reflect(ox + lx - R, W);
        tile[e] = med_key(x[base + (size_t)gy * W + gx]);
    }
    __syncthreads();
    const int lx = threadIdx.x % MED_TX, ly = threadIdx.x / MED_TX;
    unsigned v[KK];
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) v[dy * K + dx] = tile[(ly + dy) * PW + lx + dx];
    // the key of rank RANK is the largest m with #{key < m} <= RANK; the predicate is monotone in m: build m bit by bit.
    // The leading bits that all keys of the wave's windows share are the median's too: start below them (a depth map's
    // neighbouring values share sign, exponent and the first mantissa bits; a constant tile takes no step at all)
    const unsigned ref = (unsigned)__builtin_amdgcn_readfirstlane((int)v[0]);
    unsigned diff = 0u;
#pragma unroll
    for (int j = 0; j < KK; ++j) diff |= v[j] ^ ref;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) diff |= (unsigned)__shfl_xor((int)diff, s);
    diff = (unsigned)__builtin_amdgcn_readfirstlane((int)diff);
    const int top = diff ? 31 - __clz((int)diff) : -1;                  // highest bit in which two keys differ
    unsigned m = diff ? ref & ~(0xffffffffu >> __clz((int)diff)) : ref;  // the shared bits above it
#pragma unroll 1
    for (int bit = top; bit >= 0; --bit) {
        const unsigned cand = m | (1u << bit);
        int below = 0;
#pragma unroll
        for (int j = 0; j < KK; ++j) below += v[j] < cand ? 1 : 0;
        m = below <= RANK ? cand : m;
    }
    const int px = ox + lx, py = oy + ly;
    if (px < W && py < H) out[base + (size_t)py * W + px] = med_unkey(m);
}

// ---------------------------------------------------------------------------------------------------------------- lifting
constexpr int LIFT_THREADS = 256, LIFT_WAVES = LIFT_THREADS / WAVE;

// grid_sample(align_corners=True, mode="bilinear") of one channel at grid coordinates (gx, gy) in [-1, 1]; `es` = element
// stride of the image (1: a [H, W] plane, 3: one channel of an [H, W, 3] image).  BORDER: coordinates clipped to the image
// first (padding_mode="border"); otherwise corners outside the image are skipped (padding_mode="zeros").
template <bool BORDER>
__device__ __forceinline__ float bilinear(const float *__restrict__ img, int H, int W, int es, float gx, float gy) {
    const float wm = (float)(W - 1), hm = (float)(H - 1);
    float ix = ((gx + 1.f) / 2.f) * wm, iy = ((gy + 1.f) / 2.f) * hm;
    if (BORDER) {
        ix = fminf(fmaxf(ix, 0.f), wm);
        iy = fminf(fmaxf(iy, 0.f), hm);
    }
    const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.f, y1 = y0 + 1.f;
    const float nw = (x1 - ix) * (y1 - iy), ne = (ix - x0) * (y1 - iy), sw = (x1 - ix) * (iy - y0), se = (ix - x0) * (iy - y0);
    // range tests on the floats (a NaN or huge coordinate is outside): only corners inside the image are addressed
    const bool bx0 = x0 >= 0.f && x0 <= wm, bx1 = x1 >= 0.f && x1 <= wm, by0 = y0 >= 0.f && y0 <= hm, by1 = y1 >= 0.f && y1 <= hm;
    const int jx0 = bx0 ? (int)x0 : 0, jx1 = bx1 ? (int)x1 : 0, jy0 = by0 ? (int)y0 : 0, jy1 = by1 ? (int)y1 : 0;
    float acc = 0.f;
    if (bx0 && by0) acc = acc + nw * img[((size_t)jy0 * W + jx0) * es];
    if (bx1 && by0) acc = acc + ne * img[((size_t)jy0 * W + jx1) * es];
    if (bx0 && by1) acc = acc + sw * img[((size_t)jy1 * W + jx0) * es];
    if (bx1 && by1) acc = acc + se * img[((size_t)jy1 * W + jx1) * es];
    return acc;
}

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

__global__ void __launch_bounds__(LIFT_THREADS)
lift_kernel(int N, int T, int H, int W, const float4 *__restrict__ tracks, const float *__restrict__ depths,
            const float *__restrict__ masks, int query_index, const float *__restrict__ query_img, int grid_coords,
            float *__restrict__ tracks_3d, float *__restrict__ colors, unsigned char *__restrict__ visibles,
            unsigned char *__restrict__ invisibles, float *__restrict__ confidences, unsigned char *__restrict__ in_mask,
            int *__restrict__ counts) {
    const int lane = threadIdx.x & (WAVE - 1), n = blockIdx.x * LIFT_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;  // (wave-uniform)
    const size_t plane = (size_t)H * (size_t)W;
    const float half_w = (float)W / 2.f, half_h = (float)H / 2.f;
    int n_vis = 0, n_conf = 0;
    for (int t = lane; t < T; t += WAVE) {
        const size_t o = (size_t)n * T + t;
        const float4 tr = tracks[o];
        // parse_tapir_track_info (utils.py:53-66)
        const float vis = 1.f - sigmoid_f(tr.z);
        float conf = 1.f - sigmoid_f(tr.w);
        bool vv = vis * conf > 0.5f, vi = (1.f - vis) * conf > 0.5f;
        conf = conf * ((vv || vi) ? 1.f : 0.f);
        // normalize_coords (utils.py:27-29) unless the caller hands grid coordinates
        const float gx = grid_coords ? tr.x : tr.x / (float)(W - 1) * 2.f - 1.f;
        const float gy = grid_coords ? tr.y : tr.y / (float)(H - 1) * 2.f - 1.f;
        const float depth = bilinear<true>(depths + t * plane, H, W, 1, gx, gy);
        const bool in = bilinear<false>(masks + t * plane, H, W, 1, gx, gy) == 1.f;
        vv = vv && in;
        vi = vi && in;
        conf = conf * (in ? 1.f : 0.f);
        tracks_3d[3 * o] = grid_coords ? tr.x : (tr.x - half_w) / half_w;
        tracks_3d[3 * o + 1] = grid_coords ? tr.y : (tr.y - half_h) / half_h;
        tracks_3d[3 * o + 2] = depth;
        visibles[o] = vv ? 1 : 0;
        invisibles[o] = vi ? 1 : 0;
        confidences[o] = conf;
        in_mask[o] = in ? 1 : 0;
        n_vis += vv ? 1 : 0;
        n_conf += conf > 0.5f ? 1 : 0;
        if (t == query_index) {
#pragma unroll
            for (int c = 0; c < 3; ++c) colors[3 * (size_t)n + c] = bilinear<true>(query_img + c, H, W, 3, gx, gy);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {  // integer sums: exact in any order
        n_vis += __shfl_xor(n_vis, s);
        n_conf += __shfl_xor(n_conf, s);
    }
    if (lane == 0) {
        counts[2 * (size_t)n] = n_vis;
        counts[2 * (size_t)n + 1] = n_conf;
    }
}

// ---------------------------------------------------------------------------------------------------------------- spline
constexpr int SPL_THREADS = 64;
struct SplineFactor {  // Thomas factors of the knot-slope matrix (float64, host) + what the right-hand side needs
    double mul[SPLAT_SPLINE_MAX_KNOTS];    // row i: lower[i] / pivot[i-1]
    double pivot[SPLAT_SPLINE_MAX_KNOTS];  // row i: diag[i] - mul[i] * upper[i-1]
    double upper[SPLAT_SPLINE_MAX_KNOTS];
    double dx[SPLAT_SPLINE_MAX_KNOTS];     // knot spacing of segment i
    int frame[SPLAT_SPLINE_MAX_KNOTS];     // frame index of knot i
    int n;
};

// right-hand side of row i (scipy.interpolate.CubicSpline, bc_type="not-a-knot"); s0 / s1 = slopes of segments i-1 / i
// (first row: segments 0 / 1; last row: segments n-3 / n-2)
__device__ __forceinline__ double spline_rhs(const SplineFactor &f, int i, double s0, double s1) {
    const int n = f.n;
    if (n == 2) return s0;                                                         // a line: both knot slopes = its slope
    if (n == 3 && i != 1) return 2.0 * (i == 0 ? s0 : s1);                         // the parabola through three knots
    if (i == 0) {
        const double d = f.dx[0] + f.dx[1];
        return ((f.dx[0] + 2.0 * d) * f.dx[1] * s0 + f.dx[0] * f.dx[0] * s1) / d;
    }
    if (i == n - 1) {
        const double d = f.dx[n - 2] + f.dx[n - 3];
        return (f.dx[n - 2] * f.dx[n - 2] * s0 + (2.0 * d + f.dx[n - 2]) * f.dx[n - 3] * s1) / d;
    }
    return 3.0 * (f.dx[i] * s0 + f.dx[i - 1] * s1);
}

__global__ void __launch_bounds__(SPL_THREADS)
spline_kernel(int N, int T, SplineFactor f, const float *__restrict__ tracks, float *__restrict__ position,
              float *__restrict__ cubic) {
    extern __shared__ __attribute__((aligned(16))) double swept[];  // [n][SPL_THREADS]: a column per thread, 8-byte lanes side by side
    const long long g = (long long)blockIdx.x * SPL_THREADS + threadIdx.x;
    if (g >= 3ll * N) return;
    const int n = f.n, I = n - 1, c = (int)(g % 3);
    const size_t gi = (size_t)(g / 3);
    const float *tr = tracks + gi * (size_t)T * 3 + c;
    const float base = tr[0];
    position[3 * gi + c] = base;
    double *col = swept + threadIdx.x;
    // y of knot i = the track minus its frame-0 point, a float32 difference like the reference's delta_position
    auto yk = [&](int i) { return (double)(tr[3 * (size_t)f.frame[i]] - base); };
    // forward sweep; the slopes of the two segments a row needs are rebuilt from three y values on the way
    double y1 = yk(1);                                       // y of the last knot read
    double sl_prev = (y1 - yk(0)) / f.dx[0], sl = sl_prev;   // slopes of segments i-1 and i
    if (n > 2) {
        const double y2 = yk(2);
        sl = (y2 - y1) / f.dx[1];
        y1 = y2;
    }
    double carry = spline_rhs(f, 0, sl_prev, sl);
    col[0] = carry;
    for (int i = 1; i < n; ++i) {
        if (i >= 2 && i + 1 < n) {  // rows 1 .. n-2 use segments i-1, i; the last row keeps the pair of row n-2
            const double y2 = yk(i + 1);
            sl_prev = sl;
            sl = (y2 - y1) / f.dx[i];
            y1 = y2;
        }
        carry = spline_rhs(f, i, sl_prev, sl) - f.mul[i] * carry;
        col[(size_t)i * SPL_THREADS] = carry;
    }
    // back substitution; segment i is complete once the knot slopes i and i + 1 are known
    double s_hi = carry / f.pivot[n - 1];
    float *out = cubic + gi * (size_t)(12 * I) + c;  // [4, I, 3] of this Gaussian, highest power first
    for (int i = n - 2; i >= 0; --i) {
        const double s_lo = (col[(size_t)i * SPL_THREADS] - f.upper[i] * s_hi) / f.pivot[i];
        const float ya = tr[3 * (size_t)f.frame[i]] - base, yb = tr[3 * (size_t)f.frame[i + 1]] - base;
        const double h = f.dx[i], slope = ((double)yb - (double)ya) / h;
        const double tt = (s_lo + s_hi - 2.0 * slope) / h;
        out[(0 * I + i) * 3] = (float)(tt / h);
        out[(1 * I + i) * 3] = (float)((slope - s_lo) / h - tt);
        out[(2 * I + i) * 3] = (float)s_lo;
        out[(3 * I + i) * 3] = ya;
        s_hi = s_lo;
    }
}
}  // namespace

// K x K median of P planes [H, W] with reflect padding of K / 2: out = the element of rank (K*K-1)/2 of every window.
extern "C" int splat_median_filter_2d(int P, int H, int W, int k, const float *x, float *out, void *stream) {
    SPLAT_CHECK_ARG(P >= 0 && H >= 0 && W >= 0, "bad sizes");
    SPLAT_CHECK_ARG(k >= 3 && k <= 11 && (k & 1), "kernel_size must be odd, 3..11");
    if (P == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(H > k / 2 && W > k / 2, "H and W must exceed kernel_size / 2 (reflect padding)");
    const long long tiles_x = (W + MED_TX - 1) / MED_TX, tiles_y = (H + MED_TY - 1) / MED_TY;
    SPLAT_CHECK_ARG(tiles_x * tiles_y * (long long)P < (1ll << 31), "too many tiles");
    SPLAT_CHECK_ARG(x && out, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles_x * tiles_y * P)), block(MED_THREADS);
    switch (k) {
    case 3: SPLAT_LAUNCH("median_3", median_kernel<3>, grid, block, 0, s, H, W, (int)tiles_x, (int)tiles_y, x, out); break;
    case 5: SPLAT_LAUNCH("median_5", median_kernel<5>, grid, block, 0, s, H, W, (int)tiles_x, (int)tiles_y, x, out); break;
    case 7: SPLAT_LAUNCH("median_7", median_kernel<7>, grid, block, 0, s, H, W, (int)tiles_x, (int)tiles_y, x, out); break;
    case 9: SPLAT_LAUNCH("median_9", median_kernel<9>, grid, block, 0, s, H, W, (int)tiles_x, (int)tiles_y, x, out); break;
    default: SPLAT_LAUNCH("median_11", median_kernel<11>, grid, block, 0, s, H, W, (int)tiles_x, (int)tiles_y, x, out); break;
    }
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_lift_tracks(int N, int T, int H, int W, const float *tracks_2d, const float *depths, const float *masks,
                                 int query_index, const float *query_img, int grid_coords, float *tracks_3d, float *colors,
                                 uint8_t *visibles, uint8_t *invisibles, float *confidences, uint8_t *in_mask,
                                 int32_t *counts, void *stream) {
    SPLAT_CHECK_ARG(N >= 0 && T >= 0 && H >= 0 && W >= 0, "bad sizes");
    if (N == 0 || T == 0 || H == 0 || W == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(query_index >= 0 && query_index < T, "query_index outside the clip");
    SPLAT_CHECK_ARG((long long)N * T < (1ll << 31) && (long long)T * H * W < (1ll << 40), "sizes too large");
    SPLAT_CHECK_ARG(tracks_2d && depths && masks && query_img && tracks_3d && colors && visibles && invisibles && confidences &&
                        in_mask && counts, "null pointer");
    SPLAT_LAUNCH("lift_tracks", lift_kernel, dim3((unsigned)((N + LIFT_WAVES - 1) / LIFT_WAVES)), dim3(LIFT_THREADS), 0,
                 (hipStream_t)stream, N, T, H, W, (const float4 *)tracks_2d, depths, masks, query_index, query_img,
                 grid_coords ? 1 : 0, tracks_3d, colors, visibles, invisibles, confidences, in_mask, counts);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_fit_cubic_nodes(int N, int T, int n_knots, const float *knots_host, const int32_t *knot_frames_host,
                                     const float *tracks_3d, float *position, float *pos_cubic_node, void *stream) {
    SPLAT_CHECK_ARG(N >= 0 && T >= 1, "bad sizes");
    SPLAT_CHECK_ARG(n_knots >= 2, "a spline needs at least 2 knots");
    SPLAT_CHECK_ARG(n_knots <= SPLAT_SPLINE_MAX_KNOTS, "more knots than SPLAT_SPLINE_MAX_KNOTS");
    SPLAT_CHECK_ARG(knots_host && knot_frames_host, "null pointer");
    const int n = n_knots;
    SplineFactor f;
    memset(&f, 0, sizeof(f));
    f.n = n;
    for (int i = 0; i < n; ++i) {
        SPLAT_CHECK_ARG(knot_frames_host[i] >= 0 && knot_frames_host[i] < T, "knot frame index outside the clip");
        f.frame[i] = knot_frames_host[i];
        if (i + 1 < n) {
            f.dx[i] = (double)knots_host[i + 1] - (double)knots_host[i];
            SPLAT_CHECK_ARG(f.dx[i] > 0.0, "knots must be strictly increasing");
        }
    }
    // the tridiagonal matrix of the knot slopes (scipy's, row by row), factored without pivoting: its pivots are positive
    // for increasing knots (rows 1 .. n-2 are diagonally dominant; the two not-a-knot rows reduce to dx sums)
    double lower[SPLAT_SPLINE_MAX_KNOTS], diag[SPLAT_SPLINE_MAX_KNOTS];
    for (int i = 0; i < n; ++i) {
        lower[i] = 0.0;
        f.upper[i] = 0.0;
        if (n == 2) diag[i] = 1.0;
        else if (n == 3 && i != 1) {
            diag[i] = 1.0;
            (i == 0 ? f.upper[i] : lower[i]) = 1.0;
        } else if (i == 0) {
            diag[i] = f.dx[1];
            f.upper[i] = f.dx[0] + f.dx[1];
        } else if (i == n - 1) {
            diag[i] = f.dx[n - 3];
            lower[i] = f.dx[n - 2] + f.dx[n - 3];
        } else {
            lower[i] = f.dx[i];
            diag[i] = 2.0 * (f.dx[i - 1] + f.dx[i]);
            f.upper[i] = f.dx[i - 1];
        }
    }
    f.pivot[0] = diag[0];
    for (int i = 1; i < n; ++i) {
        f.mul[i] = lower[i] / f.pivot[i - 1];
        f.pivot[i] = diag[i] - f.mul[i] * f.upper[i - 1];
    }
    for (int i = 0; i < n; ++i) SPLAT_CHECK_ARG(f.pivot[i] > 0.0, "singular knot matrix");
    if (N == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(tracks_3d && position && pos_cubic_node, "null pointer");
    SPLAT_CHECK_ARG((long long)N * 3 < (1ll << 31), "too many Gaussians");
    const long long threads = 3ll * N;
    SPLAT_LAUNCH("spline_fit", spline_kernel, dim3((unsigned)((threads + SPL_THREADS - 1) / SPL_THREADS)), dim3(SPL_THREADS),
                 (size_t)n * SPL_THREADS * sizeof(double), (hipStream_t)stream, N, T, f, tracks_3d, position, pos_cubic_node);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}
