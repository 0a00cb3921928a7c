// SSIM / D-SSIM image loss on gfx950: value, gradient and the training step's L1 + D-SSIM term, each in one tiled launch
// (+ one fixed-order reduction launch for the sums).
//
// Semantics: the reference's `ssim` / `_ssim` (src/pointrix/model/loss.py:58-112): separable Gaussian window of `window` taps,
// sigma 1.5, normalised to sum 1; zero padding of window / 2 (no renormalisation at the borders); C1 = 0.01^2, C2 = 0.03^2;
// sigma^2 = E[x^2] - mu^2, sigma_xy = E[xy] - mu_x mu_y.  A "plane" is one (image, channel) pair of an [N, Cp, Hp, Wp] view
// given by four element strides per tensor, so the reference's HWC call (channel = dim -3 = the image row) and the usual
// per-colour image SSIM are the same kernels with other strides; nothing is copied.
//
// One workgroup = one output tile of one plane.  Everything a tile needs is staged in LDS and recomputed; no map goes to HBM:
//   1. the inputs x, y on the moment region + r (clipped to the plane: outside the plane is zero padding)
//   2. horizontal pass: 5 row sums (x, y, x^2, y^2, xy) on the moment region's columns
//   3. vertical pass: the 5 moments on the moment region -> SSIM (value) and, for the gradient, the per-position partials
//        B = ds/dsigma_x^2, Cm = ds/dsigma_xy, A = ds/dmu_x - 2 mu_x B - mu_y Cm   (times the upstream gradient of the map)
//      value only: moment region = output tile; gradient: output tile + r (the positions whose window covers the tile)
//   4. / 5. the same separable window over A, B, Cm (only map positions inside the plane: the transpose of the zero-padded
//      correlation) -> dS/dx(p) = blur(A) + 2 x blur(B) + y blur(Cm)
// Sums leave as one partial per workgroup; ssim_reduce_kernel adds them up in a fixed order (no float atomics: bit-reproducible).
#include "common.h"

#include <algorithm>

namespace {

constexpr int SSIM_MAX_R = 7;          // window sizes 1 .. 15 (odd)
constexpr int SSIM_THREADS = 256;
constexpr size_t SSIM_LDS_MAX = 65536;  // per workgroup: two workgroups of the largest tile share a CU's 160 KiB
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

// w[RT + j], j in [-RT, RT]; zero beyond the window's own radius (a 15-tap loop serves every smaller window)
struct SsimWin {
    float w[2 * SSIM_MAX_R + 1];
};

struct SsimImg {
    const float *p;
    long long s[4];
};

struct SsimArgs {
    int Cp, Hp, Wp, r;
    int TH, TW, tiles_x, tiles;   // tile, tiles along the plane's columns, tiles per plane
    int row_fast;                 // global accesses walk the plane's rows fastest (stride of dim 2 below that of dim 3)
    SsimImg a, b;                 // a: the image differentiated (pred); b: the other one
    float *grad;                  // gradient w.r.t. a (modes 1, 2)
    long long gs[4];
    int accumulate;
    const float *g_dev;           // mode 1: upstream gradient, device scalar or [N] (g_per_image)
    int g_per_image;
    float g_scale;                // mode 1: times g_dev; mode 2: the map's upstream gradient itself (-w_ssim / n)
    float l1_scale;               // mode 2: w_l1 / n
    float *partial;               // [blocks, 2]: sum of s, sum |a - b| over the tile (modes 0, 2)
};

// i -> (i / d, i % d) for i < 2^20 through a float reciprocal (exact there: the quotient's error stays far below 0.5 / d)
__device__ __forceinline__ void split_idx(int i, int d, float inv, int &q, int &rem) {
    q = (int)(((float)i + 0.5f) * inv);
    rem = i - q * d;
}

__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum_to_lane63(v);
    if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}

// MODE 0: value; 1: gradient of the (upstream-weighted) mean; 2: gradient of l1_scale * |a - b| + g_scale * s, with both sums
template <int RT, int MODE>
__global__ void __launch_bounds__(SSIM_THREADS) ssim_tile_kernel(SsimArgs A, SsimWin W) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr bool GRAD = MODE != 0;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int plane = b / A.tiles, t = b - plane * A.tiles;
    const int n = plane / A.Cp, c = plane - n * A.Cp;
    const int ty = t / A.tiles_x, tx = t - ty * A.tiles_x;
    const int r = A.r, Hp = A.Hp, Wp = A.Wp;
    // output tile O, moment region M (O + r for the gradient), input region I = M + r; all clipped to the plane
    const int oy0 = ty * A.TH, oy1 = imin_(oy0 + A.TH, Hp), ox0 = tx * A.TW, ox1 = imin_(ox0 + A.TW, Wp);
    const int mr = GRAD ? r : 0;
    const int my0 = imax_(oy0 - mr, 0), my1 = imin_(oy1 + mr, Hp), mx0 = imax_(ox0 - mr, 0), mx1 = imin_(ox1 + mr, Wp);
    const int iy0 = imax_(my0 - r, 0), iy1 = imin_(my1 + r, Hp), ix0 = imax_(mx0 - r, 0), ix1 = imin_(mx1 + r, Wp);
    const int ih = iy1 - iy0, iw = ix1 - ix0, mh = my1 - my0, mw = mx1 - mx0, oh = oy1 - oy0, ow = ox1 - ox0;

    float *red = sm;                           // 16 floats (4 used)
    float *X = sm + 16, *Y = X + ih * iw;       // [ih][iw]
    float *Hs = Y + ih * iw;                    // 5 planes [ih][mw]
    float *S3 = Hs + 5 * ih * mw;               // 3 planes [mh][mw] (gradient)
    float *G = Hs;                              // 3 planes [mh][ow] (gradient; H is dead by then)
    const int nH = ih * mw, nS = mh * mw, nG = mh * ow;

    const float *pa = A.a.p + (long long)n * A.a.s[0] + (long long)c * A.a.s[1];
    const float *pb = A.b.p + (long long)n * A.b.s[0] + (long long)c * A.b.s[1];

    // ---- 1. inputs of the region I
    {
        const int tot = ih * iw;
        const int d = A.row_fast ? ih : iw;
        const float inv = 1.0f / (float)d;
        for (int i = tid; i < tot; i += SSIM_THREADS) {
            int q, rem, y, x;
            split_idx(i, d, inv, q, rem);
            if (A.row_fast) { y = rem; x = q; } else { y = q; x = rem; }
            const long long ya = iy0 + y, xa = ix0 + x;
            X[y * iw + x] = pa[ya * A.a.s[2] + xa * A.a.s[3]];
            Y[y * iw + x] = pb[ya * A.b.s[2] + xa * A.b.s[3]];
        }
    }
    __syncthreads();

    // ---- 2. horizontal pass: rows of I, columns of M
    {
        const float inv = 1.0f / (float)mw;
        for (int i = tid; i < nH; i += SSIM_THREADS) {
            int y, x;
            split_idx(i, mw, inv, y, x);
            const float *xr = X + y * iw, *yr = Y + y * iw;
            const int xc = mx0 - ix0 + x;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
            for (int j = -RT; j <= RT; ++j) {
                const int q = xc + j;
                const bool ok = (unsigned)q < (unsigned)iw;
                const int qc = ok ? q : 0;
                const float u = ok ? xr[qc] : 0.f, v = ok ? yr[qc] : 0.f;
                const float w = W.w[RT + j];
                const float wu = w * u, wv = w * v;
                s0 += wu; s1 += wv; s2 += wu * u; s3 += wv * v; s4 += wu * v;
            }
            Hs[i] = s0; Hs[nH + i] = s1; Hs[2 * nH + i] = s2; Hs[3 * nH + i] = s3; Hs[4 * nH + i] = s4;
        }
    }
    __syncthreads();

    // ---- 3. vertical pass: the moments on M, SSIM and (gradient) the map partials A, B, Cm
    float acc_s = 0.f;
    {
        float gsc = 0.f;
        if (MODE == 1) gsc = A.g_scale * A.g_dev[A.g_per_image ? n : 0];
        if (MODE == 2) gsc = A.g_scale;
        const float inv = 1.0f / (float)mw;
        for (int i = tid; i < nS; i += SSIM_THREADS) {
            int y, x;
            split_idx(i, mw, inv, y, x);
            const int yc = my0 - iy0 + y;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int j = -RT; j <= RT; ++j) {
                const int q = yc + j;
                const bool ok = (unsigned)q < (unsigned)ih;
                const int k = (ok ? q : 0) * mw + x;
                const float w = ok ? W.w[RT + j] : 0.f;
                m0 += w * Hs[k]; m1 += w * Hs[nH + k]; m2 += w * Hs[2 * nH + k]; m3 += w * Hs[3 * nH + k];
                m4 += w * Hs[4 * nH + k];
            }
            const float mu1_sq = m0 * m0, mu2_sq = m1 * m1, mu12 = m0 * m1;
            const float s1sq = m2 - mu1_sq, s2sq = m3 - mu2_sq, s12 = m4 - mu12;
            const float a1 = 2.f * mu12 + SSIM_C1, a2 = 2.f * s12 + SSIM_C2;
            const float b1 = mu1_sq + mu2_sq + SSIM_C1, b2 = s1sq + s2sq + SSIM_C2;
            const float den = b1 * b2;
            const float s = (a1 * a2) / den;
            const int ya = my0 + y, xa = mx0 + x;
            if (MODE != 1 && ya >= oy0 && ya < oy1 && xa >= ox0 && xa < ox1) acc_s += s;
            if (GRAD) {
                const float rden = 1.f / den;
                const float Bv = -s / b2;
                const float Cv = 2.f * a1 * rden;
                const float dmu = 2.f * m1 * a2 * rden - 2.f * m0 * s / b1;
                const float Av = dmu - 2.f * m0 * Bv - m1 * Cv;
                S3[i] = gsc * Av; S3[nS + i] = gsc * Bv; S3[2 * nS + i] = gsc * Cv;
            }
        }
    }

    float acc_l1 = 0.f;
    if (GRAD) {
        __syncthreads();
        // ---- 4. horizontal blur of A, B, Cm: rows of M, columns of O
        {
            const float inv = 1.0f / (float)ow;
            for (int i = tid; i < nG; i += SSIM_THREADS) {
                int y, x;
                split_idx(i, ow, inv, y, x);
                const float *r0 = S3 + y * mw;
                const int xc = ox0 - mx0 + x;
                float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
                for (int j = -RT; j <= RT; ++j) {
                    const int q = xc + j;
                    const bool ok = (unsigned)q < (unsigned)mw;
                    const int qc = ok ? q : 0;
                    const float w = ok ? W.w[RT + j] : 0.f;
                    g0 += w * r0[qc]; g1 += w * r0[nS + qc]; g2 += w * r0[2 * nS + qc];
                }
                G[i] = g0; G[nG + i] = g1; G[2 * nG + i] = g2;
            }
        }
        __syncthreads();
        // ---- 5. vertical blur on O, the gradient (and the L1 term)
        {
            const int tot = oh * ow;
            const int d = A.row_fast ? oh : ow;
            const float inv = 1.0f / (float)d;
            float *pg = A.grad + (long long)n * A.gs[0] + (long long)c * A.gs[1];
            for (int i = tid; i < tot; i += SSIM_THREADS) {
                int q0, rem, y, x;
                split_idx(i, d, inv, q0, rem);
                if (A.row_fast) { y = rem; x = q0; } else { y = q0; x = rem; }
                const int yc = oy0 - my0 + y;
                float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
                for (int j = -RT; j <= RT; ++j) {
                    const int q = yc + j;
                    const bool ok = (unsigned)q < (unsigned)mh;
                    const int k = (ok ? q : 0) * ow + x;
                    const float w = ok ? W.w[RT + j] : 0.f;
                    g0 += w * G[k]; g1 += w * G[nG + k]; g2 += w * G[2 * nG + k];
                }
                const int li = (oy0 - iy0 + y) * iw + (ox0 - ix0 + x);
                const float u = X[li], v = Y[li];
                float g = g0 + 2.f * u * g1 + v * g2;
                if (MODE == 2) {
                    const float dl = u - v;
                    acc_l1 += fabsf(dl);
                    g += dl > 0.f ? A.l1_scale : (dl < 0.f ? -A.l1_scale : 0.f);
                }
                float *dst = pg + (long long)(oy0 + y) * A.gs[2] + (long long)(ox0 + x) * A.gs[3];
                *dst = A.accumulate ? *dst + g : g;
            }
        }
    }

    if (MODE != 1) {
        const float ts = block_sum(acc_s, red);
        const float tl = MODE == 2 ? block_sum(acc_l1, red) : 0.f;
        if (tid == 0) {
            A.partial[2 * (long long)b] = ts;
            A.partial[2 * (long long)b + 1] = tl;
        }
    }
}

// the per-workgroup partials of image n are blocks [n * bpi, (n + 1) * bpi): per-image means, the overall mean, and the sums
// ADDED into the caller's slots -- one workgroup, a fixed order of additions
__global__ void __launch_bounds__(SSIM_THREADS)
ssim_reduce_kernel(int N, int bpi, const float *__restrict__ partial, float inv_count, float inv_total, float *mean,
                   float *per_image, float *s_slot, float *l1_slot) {
    __shared__ float red[16];
    float tot_s = 0.f, tot_l = 0.f;
    for (int n = 0; n < N; ++n) {
        const float *p = partial + 2 * (long long)n * bpi;
        float s = 0.f, l = 0.f;
        for (int k = threadIdx.x; k < bpi; k += SSIM_THREADS) {
            s += p[2 * k];
            l += p[2 * k + 1];
        }
        s = block_sum(s, red);
        l = block_sum(l, red);
        if (threadIdx.x == 0) {
            if (per_image) per_image[n] = s * inv_count;
            tot_s += s;
            tot_l += l;
        }
    }
    if (threadIdx.x == 0) {
        if (mean) *mean = tot_s * inv_total;
        if (s_slot) *s_slot += tot_s;
        if (l1_slot) *l1_slot += tot_l;
    }
}

struct SsimPlan {
    int TH, TW, tiles_x, tiles, blocks, bpi, r, RT;
    size_t lds;
};

// LDS of a tile (upper bound over the plane's tiles: every region is clipped to the plane)
size_t ssim_lds_bytes(bool grad, int TH, int TW, int Hp, int Wp, int r) {
    const int mr = grad ? r : 0;
    const long long mh = std::min(TH + 2 * mr, Hp), mw = std::min(TW + 2 * mr, Wp);
    const long long ih = std::min((int)mh + 2 * r, Hp), iw = std::min((int)mw + 2 * r, Wp);
    long long f = 16 + 2 * ih * iw + 5 * ih * mw;
    if (grad) f += 3 * mh * mw;
    return (size_t)f * sizeof(float);
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// tile by plane shape: narrow planes (<= 8 columns, the reference's 854 x 3 HWC planes) as column strips of whole width,
// flat ones (<= 8 rows) as row strips, the rest as 2-D tiles; tiles balanced over the plane, sized for the gradient's LDS
// (the value kernel uses the same tiles, so one scratch size serves every entry point)
bool ssim_plan(int N, int Cp, int Hp, int Wp, int window, SsimPlan &P) {
    P.r = window / 2;
    P.RT = P.r <= 5 ? 5 : SSIM_MAX_R;
    int thmax, twmax;
    if (Wp <= 8) { thmax = 512; twmax = Wp; }
    else if (Hp <= 8) { thmax = Hp; twmax = 512; }
    else if (P.RT == 5) { thmax = 16; twmax = 32; }
    else { thmax = 16; twmax = 16; }
    for (;;) {
        P.TH = ceil_div(Hp, ceil_div(Hp, thmax));
        P.TW = ceil_div(Wp, ceil_div(Wp, twmax));
        P.lds = ssim_lds_bytes(true, P.TH, P.TW, Hp, Wp, P.r);
        if (P.lds <= SSIM_LDS_MAX) break;
        if (thmax >= twmax && thmax > 1) thmax = (thmax + 1) / 2;
        else if (twmax > 1) twmax = (twmax + 1) / 2;
        else return false;
    }
    P.tiles_x = ceil_div(Wp, P.TW);
    const long long tiles = (long long)ceil_div(Hp, P.TH) * P.tiles_x;
    const long long bpi = tiles * Cp, blocks = bpi * N;
    if (blocks > 0x7fffffffLL) return false;
    P.tiles = (int)tiles;
    P.bpi = (int)bpi;
    P.blocks = (int)blocks;
    return true;
}

// the reference's window (gaussian(window_size, 1.5): float32 values normalised by their float32 sum), at RT + j
SsimWin ssim_window(int window, int RT) {
    SsimWin W;
    for (int k = 0; k < 2 * SSIM_MAX_R + 1; ++k) W.w[k] = 0.f;
    const int r = window / 2;
    float g[2 * SSIM_MAX_R + 1], sum = 0.f;
    for (int x = 0; x < window; ++x) {
        g[x] = (float)exp(-(double)((x - r) * (x - r)) / (2.0 * 1.5 * 1.5));
        sum += g[x];
    }
    for (int x = 0; x < window; ++x) W.w[RT + x - r] = g[x] / sum;
    return W;
}

int ssim_check_common(int N, int Cp, int Hp, int Wp, int window, const float *img1, const int64_t *s1, const float *img2,
                      const int64_t *s2, SsimPlan &P) {
    SPLAT_CHECK_ARG(N >= 1 && Cp >= 1 && Hp >= 1 && Wp >= 1, "bad sizes (every size must be >= 1)");
    SPLAT_CHECK_ARG(window >= 1 && window <= 2 * SSIM_MAX_R + 1 && (window & 1), "window must be odd, 1 .. 15");
    SPLAT_CHECK_ARG(img1 && img2 && s1 && s2, "null pointer");
    for (int k = 0; k < 4; ++k) SPLAT_CHECK_ARG(s1[k] >= 0 && s2[k] >= 0, "strides must be >= 0");
    SPLAT_CHECK_ARG(ssim_plan(N, Cp, Hp, Wp, window, P), "too many planes / tiles");
    return SPLAT_OK;
}

SsimArgs ssim_args(int Cp, int Hp, int Wp, const SsimPlan &P, const float *a, const int64_t *sa, const float *b,
                   const int64_t *sb) {
    SsimArgs A;
    memset(&A, 0, sizeof(A));
    A.Cp = Cp; A.Hp = Hp; A.Wp = Wp; A.r = P.r;
    A.TH = P.TH; A.TW = P.TW; A.tiles_x = P.tiles_x; A.tiles = P.tiles;
    A.a.p = a; A.b.p = b;
    for (int k = 0; k < 4; ++k) { A.a.s[k] = sa[k]; A.b.s[k] = sb[k]; }
    A.row_fast = sa[2] < sa[3];
    return A;
}

template <int MODE>
void ssim_launch(const SsimPlan &P, const SsimArgs &A, const SsimWin &W, hipStream_t s) {
    const size_t lds = MODE == 0 ? ssim_lds_bytes(false, P.TH, P.TW, A.Hp, A.Wp, P.r) : P.lds;
    if (P.RT == 5)
        SPLAT_LAUNCH("ssim_tile", (ssim_tile_kernel<5, MODE>), dim3(P.blocks), dim3(SSIM_THREADS), lds, s, A, W);
    else
        SPLAT_LAUNCH("ssim_tile", (ssim_tile_kernel<SSIM_MAX_R, MODE>), dim3(P.blocks), dim3(SSIM_THREADS), lds, s, A, W);
}

}  // namespace

extern "C" size_t splat_ssim_scratch_bytes(int N, int Cp, int Hp, int Wp, int window) {
    SsimPlan P;
    if (N < 1 || Cp < 1 || Hp < 1 || Wp < 1 || window < 1 || window > 2 * SSIM_MAX_R + 1 || !(window & 1)) return 0;
    if (!ssim_plan(N, Cp, Hp, Wp, window, P)) return 0;
    return ((size_t)P.blocks * 2 * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int splat_ssim_forward(int N, int Cp, int Hp, int Wp, int window, const float *img1, const int64_t *strides1,
                                  const float *img2, const int64_t *strides2, float *out_mean, float *out_per_image,
                                  void *scratch, splat_stream_t stream) {
    SsimPlan P;
    const int rc = ssim_check_common(N, Cp, Hp, Wp, window, img1, strides1, img2, strides2, P);
    if (rc) return rc;
    SPLAT_CHECK_ARG(scratch && (out_mean || out_per_image), "null pointer (scratch, or both outputs)");
    SsimArgs A = ssim_args(Cp, Hp, Wp, P, img1, strides1, img2, strides2);
    A.partial = (float *)scratch;
    const SsimWin W = ssim_window(window, P.RT);
    ssim_launch<0>(P, A, W, (hipStream_t)stream);
    SPLAT_POST_LAUNCH();
    const double count = (double)Cp * Hp * Wp;
    SPLAT_LAUNCH("ssim_reduce", ssim_reduce_kernel, dim3(1), dim3(SSIM_THREADS), 0, (hipStream_t)stream, N, P.bpi,
                 (const float *)scratch, (float)(1.0 / count), (float)(1.0 / (count * N)), out_mean, out_per_image,
                 (float *)nullptr, (float *)nullptr);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_ssim_backward(int N, int Cp, int Hp, int Wp, int window, const float *img1, const int64_t *strides1,
                                   const float *img2, const int64_t *strides2, const float *grad_out, int per_image,
                                   float *grad1, const int64_t *grad_strides, int accumulate, splat_stream_t stream) {
    SsimPlan P;
    const int rc = ssim_check_common(N, Cp, Hp, Wp, window, img1, strides1, img2, strides2, P);
    if (rc) return rc;
    SPLAT_CHECK_ARG(grad_out && grad1 && grad_strides, "null pointer");
    for (int k = 0; k < 4; ++k) SPLAT_CHECK_ARG(grad_strides[k] >= 0, "strides must be >= 0");
    SsimArgs A = ssim_args(Cp, Hp, Wp, P, img1, strides1, img2, strides2);
    A.grad = grad1;
    for (int k = 0; k < 4; ++k) A.gs[k] = grad_strides[k];
    A.accumulate = accumulate ? 1 : 0;
    A.g_dev = grad_out;
    A.g_per_image = per_image ? 1 : 0;
    A.g_scale = (float)(1.0 / ((double)Cp * Hp * Wp * (per_image ? 1 : N)));
    const SsimWin W = ssim_window(window, P.RT);
    ssim_launch<1>(P, A, W, (hipStream_t)stream);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_dssim_l1_loss_grad(int N, int Cp, int Hp, int Wp, int window, const float *pred,
                                        const int64_t *pred_strides, const float *gt, const int64_t *gt_strides, float w_l1,
                                        float w_ssim, float *grad, const int64_t *grad_strides, float *l1_sum,
                                        float *ssim_sum, void *scratch, splat_stream_t stream) {
    SsimPlan P;
    const int rc = ssim_check_common(N, Cp, Hp, Wp, window, pred, pred_strides, gt, gt_strides, P);
    if (rc) return rc;
    SPLAT_CHECK_ARG(grad && grad_strides && scratch, "null pointer");
    for (int k = 0; k < 4; ++k) SPLAT_CHECK_ARG(grad_strides[k] >= 0, "strides must be >= 0");
    SsimArgs A = ssim_args(Cp, Hp, Wp, P, pred, pred_strides, gt, gt_strides);
    const double n = (double)N * Cp * Hp * Wp;
    A.grad = grad;
    for (int k = 0; k < 4; ++k) A.gs[k] = grad_strides[k];
    A.g_scale = (float)(-(double)w_ssim / n);
    A.l1_scale = (float)((double)w_l1 / n);
    A.partial = (float *)scratch;
    const SsimWin W = ssim_window(window, P.RT);
    ssim_launch<2>(P, A, W, (hipStream_t)stream);
    SPLAT_POST_LAUNCH();
    if (l1_sum || ssim_sum) {
        SPLAT_LAUNCH("ssim_reduce", ssim_reduce_kernel, dim3(1), dim3(SSIM_THREADS), 0, (hipStream_t)stream, N, P.bpi,
                     (const float *)scratch, 0.f, 0.f, (float *)nullptr, (float *)nullptr, ssim_sum, l1_sum);
        SPLAT_POST_LAUNCH();
    }
    return SPLAT_OK;
}

// ==================================================================================================================================
// 2-D track loss: the trainer's optical-flow term on the rendered track_gs (src/trainer_fragGS.py:528-569).  Per frame f (one
// workgroup of 1024 threads):
//   1. every query e of the frame: visible when (1 - sigmoid(occ)) (1 - sigmoid(dist)) > 0.5 (parse_tapir_track_info); then
//      X = ((img[0, p] + 1) W) / 2, Y = ((img[1, p] + 1) H) / 2 (util.denormalize_coords), r = (|X - tx| + |Y - ty|) / 2 and its
//      float bits go to scratch as a uint32 key (r >= 0: the bits order as the values); invisible / malformed queries get
//      TRK_NONE, above every key.  n = the visible count.  Malformed: a pixel index out of range, or not above the frame's
//      previous one (the indices must ascend strictly, so no two queries of a frame share a pixel: the gradient's plain
//      read-modify-write never races)
//   2. radix select of rank k = floor(q (n - 1)) with four 8-bit LDS histograms, rank k + 1 by one more pass (count <= s_k,
//      min > s_k); the threshold is torch.quantile's lerp in its float32 FMA form.  A NaN residual makes torch.quantile NaN:
//      then thr = NaN, S is empty and the frame's loss is 0, as the reference's masked_l1_loss gives
//   3. sums of c r and of c over S = {r <= thr}, c = (1 - sigmoid(dist)) w_f, per thread in a fixed order + a fixed-order
//      workgroup sum; loss_f = sum c r / (sum c + 1e-8) / max(H, W) -- the trainer's masked_l1_loss(..., mask=c, quantile)
//      with its default normalize=True, divided by max(h, w)
//   4. the sparse gradient at the selected pixels (channels 0 and 1)
// The scratch keys stay in L2 (100 KB at 25.6k queries).  No float atomics (LDS integer histograms only): bit-reproducible; n
// and k never leave the device.  The residuals are computed with contraction off, so they are bit-equal to the float32 torch
// ops they restate and the selected set can be compared exactly.
namespace {

constexpr int TRK_THREADS = 1024;
constexpr unsigned TRK_NONE = 0xffffffffu;

struct TrackArgs {
    int H, W;
    const float *img;
    long long is[4];
    const int64_t *offsets;
    const int32_t *pixels;
    const float4 *targets;
    long long Q;
    const float *fw;
    float q, gscale;              // quantile; gradient weight per frame (scale / F)
    float *grad;
    long long gs[4];
    float *per_frame, *part;      // per_frame: optional output; part: scratch [F] for the slot's sum
    int32_t *counts;
    unsigned *keys;
};

__device__ __forceinline__ float trk_one_minus_sigmoid(float x) {
#pragma clang fp contract(off)
    return 1.f - 1.f / (1.f + expf(-x));
}

// query e of frame f (whose queries start at o0): false when invisible or malformed (pixel out of range, or not above the
// previous query's); else its residual parts and weight.  PTS (splat_track_loss_grad_points): the prediction is row e of a value
// table [Q, C] (is[0] = C, is[1] = 1) instead of the image's pixel -- the only difference, the pixel still decides `malformed`
template <bool PTS>
__device__ __forceinline__ bool trk_point(const TrackArgs &A, int f, long long o0, long long e, float w, float &dx, float &dy,
                                          float &r, float &c, int &py, int &px) {
#pragma clang fp contract(off)
    const int p = A.pixels[e];
    if (p < 0 || p >= A.H * A.W || (e > o0 && A.pixels[e - 1] >= p)) return false;
    const float4 t = A.targets[e];
    const float conf = trk_one_minus_sigmoid(t.w);
    if (!(trk_one_minus_sigmoid(t.z) * conf > 0.5f)) return false;
    py = p / A.W;
    px = p - py * A.W;
    const float *b = PTS ? A.img + e * A.is[0] : A.img + (long long)f * A.is[0] + (long long)py * A.is[2] + (long long)px * A.is[3];
    const float X = ((b[0] + 1.f) * (float)A.W) / 2.f;
    const float Y = ((b[A.is[1]] + 1.f) * (float)A.H) / 2.f;
    dx = X - t.x;
    dy = Y - t.y;
    r = (fabsf(dx) + fabsf(dy)) / 2.f;
    c = conf * w;
    return true;
}

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = umin_(v, __shfl_xor(v, o));
    return v;
}

template <bool PTS>
__global__ void __launch_bounds__(TRK_THREADS) track_loss_kernel(TrackArgs A) {
#pragma clang fp contract(off)
    __shared__ unsigned hist[256];
    __shared__ unsigned su[4];
    __shared__ float red[2][TRK_THREADS / WAVE];
    __shared__ float sden;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    long long o0 = A.offsets[f], o1 = A.offsets[f + 1];
    if (!(0 <= o0 && o0 <= o1 && o1 <= A.Q)) o0 = o1 = 0;      // malformed offsets: an empty frame
    const float w = A.fw[f];
    const float maxhw = (float)(A.H > A.W ? A.H : A.W);

    // ---- 1. keys, visible count, NaN residuals
    if (tid == 0) { su[0] = 0; su[3] = 0; }
    __syncthreads();
    unsigned nloc = 0, nnan = 0;
    for (long long e = o0 + tid; e < o1; e += TRK_THREADS) {
        float dx, dy, r, c;
        int py, px;
        unsigned key = TRK_NONE;
        if (trk_point<PTS>(A, f, o0, e, w, dx, dy, r, c, py, px)) {
            key = __float_as_uint(r);
            ++nloc;
            nnan += key > 0x7f800000u;
        }
        A.keys[e] = key;
    }
    nloc = wave_sum_u(nloc);
    nnan = wave_sum_u(nnan);
    if (lane == 0) {
        atomicAdd(&su[0], nloc);
        atomicAdd(&su[3], nnan);
    }
    __syncthreads();
    const int n = (int)su[0];
    const bool has_nan = su[3] != 0;
    if (n == 0) {
        if (tid == 0) {
            if (A.per_frame) A.per_frame[f] = 0.f;
            A.part[f] = 0.f;
            if (A.counts) { A.counts[2 * f] = 0; A.counts[2 * f + 1] = 0; }
        }
        return;
    }

    // ---- 2. ranks k and k + 1 of the visible residuals, threshold (NaN when a residual is)
    float thr = __builtin_nanf("");
    if (!has_nan) {
        const float pos = A.q * (float)(n - 1);
        int k = (int)floorf(pos);
        k = k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
        const float wgt = pos - (float)k;
        unsigned prefix = 0, pmask = 0, kk = (unsigned)k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (long long e = o0 + tid; e < o1; e += TRK_THREADS) {
                const unsigned key = A.keys[e];
                if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < WAVE) {     // lane l owns bins 4l .. 4l + 3; the lane whose range holds rank kk finds the bin
                const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
                const unsigned s = (h0 + h1) + (h2 + h3);
                unsigned incl = s;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const unsigned t = __shfl_up(incl, o);
                    if (tid >= o) incl += t;
                }
                const unsigned excl = incl - s;
                if (excl <= kk && kk < incl) {
                    unsigned below = excl, b = 4 * tid;
                    if (below + h0 <= kk) { below += h0; ++b;
                        if (below + h1 <= kk) { below += h1; ++b;
                            if (below + h2 <= kk) { below += h2; ++b; } } }
                    su[1] = b;
                    su[2] = below;
                }
            }
            __syncthreads();
            prefix |= su[1] << shift;
            pmask |= 0xffu << shift;
            kk -= su[2];
            __syncthreads();
        }
        const unsigned sk = prefix;
        if (tid == 0) { su[1] = 0; su[2] = TRK_NONE; }
        __syncthreads();
        {
            unsigned cle = 0, mgt = TRK_NONE;
            for (long long e = o0 + tid; e < o1; e += TRK_THREADS) {
                const unsigned key = A.keys[e];
                if (key <= sk) ++cle;
                else mgt = umin_(mgt, key);
            }
            cle = wave_sum_u(cle);
            mgt = wave_min_u(mgt);
            if (lane == 0) {
                atomicAdd(&su[1], cle);
                atomicMin(&su[2], mgt);
            }
        }
        __syncthreads();
        const unsigned sk1 = (k + 1 >= n || su[1] >= (unsigned)k + 2u) ? sk : su[2];
        const float a = __uint_as_float(sk), b = __uint_as_float(sk1), d = b - a;
        thr = fabsf(wgt) < 0.5f ? fmaf(wgt, d, a) : fmaf(wgt - 1.f, d, b);
    }

    // ---- 3. sums of c r and of c over the selected set, |S|
    float acc = 0.f, accc = 0.f;
    unsigned sel = 0;
    for (long long e = o0 + tid; e < o1; e += TRK_THREADS) {
        const unsigned key = A.keys[e];
        if (key == TRK_NONE) continue;
        const float r = __uint_as_float(key);
        if (!(r <= thr)) continue;
        const float c = trk_one_minus_sigmoid(A.targets[e].w) * w;
        acc += c * r;
        accc += c;
        ++sel;
    }
    acc = wave_sum_to_lane63(acc);
    accc = wave_sum_to_lane63(accc);
    sel = wave_sum_u(sel);
    if (lane == WAVE - 1) {
        red[0][wv] = acc;
        red[1][wv] = accc;
    }
    __syncthreads();           // su[3] (the NaN count) was read by every thread before the passes' barriers
    if (tid == 0) su[3] = 0;
    __syncthreads();
    if (lane == 0) atomicAdd(&su[3], sel);
    __syncthreads();
    const unsigned nsel = su[3];
    if (tid == 0) {
        float s = 0.f, sc = 0.f;
        for (int i = 0; i < TRK_THREADS / WAVE; ++i) {
            s += red[0][i];
            sc += red[1][i];
        }
        const float den = sc + 1e-8f;          // ndim (= 1) * sum_S c + 1e-8 (masked_l1_loss, normalize=True)
        const float loss = (s / den) / maxhw;
        sden = den;
        if (A.per_frame) A.per_frame[f] = loss;
        A.part[f] = loss;
        if (A.counts) { A.counts[2 * f] = n; A.counts[2 * f + 1] = (int)nsel; }
    }
    if (!A.grad || nsel == 0) return;
    __syncthreads();

    // ---- 4. d(gscale * loss_f)/d img at the selected pixels: c / ((sum_S c + 1e-8) max(H, W)) / 2 * sign(d) * (W or H) / 2
    const float base = A.gscale / (sden * maxhw) * 0.5f;
    const float hx = 0.5f * (float)A.W, hy = 0.5f * (float)A.H;
    for (long long e = o0 + tid; e < o1; e += TRK_THREADS) {
        float dx, dy, r, c;
        int py, px;
        if (!trk_point<PTS>(A, f, o0, e, w, dx, dy, r, c, py, px) || !(r <= thr)) continue;
        const float g = base * c;
        float *gp = PTS ? A.grad + e * A.gs[0] : A.grad + (long long)f * A.gs[0] + (long long)py * A.gs[2] + (long long)px * A.gs[3];
        gp[0] += dx > 0.f ? g * hx : (dx < 0.f ? -(g * hx) : 0.f);
        gp[A.gs[1]] += dy > 0.f ? g * hy : (dy < 0.f ? -(g * hy) : 0.f);
    }
}

// zero the gradient image [F, C, H, W] (its own strides) before the sparse entries land; grid.y walks the planes
__global__ void __launch_bounds__(256) track_grad_zero_kernel(float *g, long long s0, long long s1, long long s2, long long s3, int C,
                                                              int H, int W, int planes) {
    const int hw = H * W;
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        float *gp = g + (long long)(pl / C) * s0 + (long long)(pl % C) * s1;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
            const int y = i / W, x = i - y * W;
            gp[(long long)y * s2 + (long long)x * s3] = 0.f;
        }
    }
}

// *slot += the mean of the per-frame losses, added in frame order
__global__ void track_loss_slot_kernel(int F, const float *part, float *slot) {
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int f = 0; f < F; ++f) s += part[f];
        *slot += s / (float)F;
    }
}

size_t trk_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t splat_track_loss_scratch_bytes(int F, int64_t Q) {
    if (F < 1 || Q < 0 || Q > 0x7fffffffLL) return 0;
    return trk_align((size_t)Q * sizeof(unsigned)) + trk_align((size_t)F * sizeof(float));
}

extern "C" int splat_track_loss_grad(int F, int H, int W, int C, const float *track, const int64_t *track_strides,
                                     const int64_t *offsets, const int32_t *pixels, const float *targets, int64_t Q,
                                     const float *frame_weights, float quantile, float scale, float *grad,
                                     const int64_t *grad_strides, int accumulate, float *per_frame, float *loss_slot,
                                     int32_t *counts, void *scratch, splat_stream_t stream) {
    SPLAT_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && C >= 2 && Q >= 0, "bad sizes (F, H, W >= 1, C >= 2, Q >= 0)");
    SPLAT_CHECK_ARG((long long)H * W <= 0x7fffffffLL && Q <= 0x7fffffffLL && F <= (1 << 24) && (long long)F * C <= 0x7fffffffLL,
                    "sizes too large");
    SPLAT_CHECK_ARG(quantile >= 0.f && quantile <= 1.f, "quantile must be in [0, 1]");
    SPLAT_CHECK_ARG(track && track_strides && offsets && frame_weights && scratch, "null pointer");
    SPLAT_CHECK_ARG(Q == 0 || (pixels && targets), "null pointer (pixels / targets)");
    SPLAT_CHECK_ARG(((uintptr_t)targets & 15) == 0, "targets must be 16-byte aligned [Q, 4] float32");
    for (int k = 0; k < 4; ++k) SPLAT_CHECK_ARG(track_strides[k] >= 0, "strides must be >= 0");
    if (grad) {
        SPLAT_CHECK_ARG(grad_strides, "null pointer (grad_strides)");
        for (int k = 0; k < 4; ++k) SPLAT_CHECK_ARG(grad_strides[k] >= 0, "strides must be >= 0");
    }
    const hipStream_t s = (hipStream_t)stream;
    TrackArgs A;
    memset(&A, 0, sizeof(A));
    A.H = H; A.W = W;
    A.img = track;
    for (int k = 0; k < 4; ++k) A.is[k] = track_strides[k];
    A.offsets = offsets; A.pixels = pixels; A.targets = (const float4 *)targets; A.Q = Q;
    A.fw = frame_weights;
    A.q = quantile;
    A.gscale = scale / (float)F;
    A.grad = grad;
    if (grad) for (int k = 0; k < 4; ++k) A.gs[k] = grad_strides[k];
    A.per_frame = per_frame;
    A.counts = counts;
    A.keys = (unsigned *)scratch;
    A.part = (float *)((char *)scratch + trk_align((size_t)Q * sizeof(unsigned)));
    if (grad && !accumulate) {
        const long long planes = (long long)F * C, hw = (long long)H * W;
        long long bx = (hw + 255) / 256;
        if (bx > 64) bx = 64;
        const unsigned by = (unsigned)(planes < 65535 ? planes : 65535);
        SPLAT_LAUNCH("track_grad_zero", track_grad_zero_kernel, dim3((unsigned)bx, by), dim3(256), 0, s, grad,
                     (long long)grad_strides[0], (long long)grad_strides[1], (long long)grad_strides[2], (long long)grad_strides[3],
                     C, H, W, (int)planes);
        SPLAT_POST_LAUNCH();
    }
    SPLAT_LAUNCH("track_loss", track_loss_kernel<false>, dim3(F), dim3(TRK_THREADS), 0, s, A);
    SPLAT_POST_LAUNCH();
    if (loss_slot) {
        SPLAT_LAUNCH("track_loss_slot", track_loss_slot_kernel, dim3(1), dim3(WAVE), 0, s, F, (const float *)A.part, loss_slot);
        SPLAT_POST_LAUNCH();
    }
    return SPLAT_OK;
}

// The same loss on PER-QUERY values: row i of values [Q, C] is the prediction of query i (what the sparse compositing returns at
// the query pixels, in target order), grad [Q, C] its gradient.  Same kernels, same contraction-off residual arithmetic: only
// the two address computations differ, so losses, counts and gradient rows are bit-equal to splat_track_loss_grad on an image
// that holds those values at the query pixels.
extern "C" int splat_track_loss_grad_points(int F, int H, int W, int C, const float *values, const int64_t *offsets,
                                            const int32_t *pixels, const float *targets, int64_t Q, const float *frame_weights,
                                            float quantile, float scale, float *grad, float *per_frame, float *loss_slot,
                                            int32_t *counts, void *scratch, splat_stream_t stream) {
    SPLAT_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && C >= 2 && Q >= 0, "bad sizes (F, H, W >= 1, C >= 2, Q >= 0)");
    SPLAT_CHECK_ARG((long long)H * W <= 0x7fffffffLL && Q <= 0x7fffffffLL && F <= (1 << 24) && (long long)Q * C <= 0x7fffffffLL,
                    "sizes too large");
    SPLAT_CHECK_ARG(quantile >= 0.f && quantile <= 1.f, "quantile must be in [0, 1]");
    SPLAT_CHECK_ARG(offsets && frame_weights && scratch, "null pointer");
    SPLAT_CHECK_ARG(Q == 0 || (values && pixels && targets), "null pointer (values / pixels / targets)");
    SPLAT_CHECK_ARG(((uintptr_t)targets & 15) == 0, "targets must be 16-byte aligned [Q, 4] float32");
    const hipStream_t s = (hipStream_t)stream;
    TrackArgs A;
    memset(&A, 0, sizeof(A));
    A.H = H; A.W = W;
    A.img = values;
    A.is[0] = C; A.is[1] = 1;
    A.offsets = offsets; A.pixels = pixels; A.targets = (const float4 *)targets; A.Q = Q;
    A.fw = frame_weights;
    A.q = quantile;
    A.gscale = scale / (float)F;
    A.grad = Q > 0 ? grad : nullptr;
    A.gs[0] = C; A.gs[1] = 1;
    A.per_frame = per_frame;
    A.counts = counts;
    A.keys = (unsigned *)scratch;
    A.part = (float *)((char *)scratch + trk_align((size_t)Q * sizeof(unsigned)));
    if (A.grad) {   // written in full: zeros outside the selected set and in channels >= 2
        const long long n = (long long)Q * C;
        long long bx = (n + 255) / 256;
        if (bx > 1024) bx = 1024;
        SPLAT_LAUNCH("track_grad_zero", track_grad_zero_kernel, dim3((unsigned)bx, 1u), dim3(256), 0, s, grad, 0ll, 0ll, 0ll, 1ll, 1, 1,
                     (int)n, 1);
        SPLAT_POST_LAUNCH();
    }
    SPLAT_LAUNCH("track_loss", track_loss_kernel<true>, dim3(F), dim3(TRK_THREADS), 0, s, A);
    SPLAT_POST_LAUNCH();
    if (loss_slot) {
        SPLAT_LAUNCH("track_loss_slot", track_loss_slot_kernel, dim3(1), dim3(WAVE), 0, s, F, (const float *)A.part, loss_slot);
        SPLAT_POST_LAUNCH();
    }
    return SPLAT_OK;
}

// ==================================================================================================================================
// Median-normalised depth loss: the trainer's depth_loss_dpt (src/loss.py:184-207, src/trainer_fragGS.py:589-601).  A "row" is one
// image of n = H W pixels: rows 0 .. F-1 are the frames of pred, rows F .. 2F-1 those of gt (absent when the caller hands in
// gt's statistics).  One workgroup = DPT_CH consecutive pixels of one row; the grid is (chunks, rows).  Launches:
//   0.     one memset of the rows' histograms and integer counters
//   1.-4.  digit pass d = 0 .. 3 of the radix select of rank (n - 1) / 2 on sign-flipped keys: every workgroup first finds the
//          bins of the digits already counted (one wave, a prefix scan over 256 counters per digit), then counts digit d of the
//          keys that match them in per-wave LDS histograms and flushes those with integer atomics; pass 0 also counts NaNs
//   5.     t from the four histograms; per workgroup the partial of sum |p - t|, and m = #{p == t}, #{p > t}, #{p < t}
//          (integer atomics)
//   6.     s = the partials added in chunk order / n; per workgroup the partials of sum d^2, sum d, sum d (p - t_p)
//   7.     those added in chunk order -> loss_f, A, B; the gradient, elementwise
//   8.     the slot: the per-frame losses added in frame order
// Partials are doubles in a fixed slot; every reader adds them in the same order: no float atomics, bit-reproducible.  What a
// launch reads of another's output crosses a kernel boundary, never a fence inside a launch.
namespace {

constexpr int DPT_THREADS = 256;
constexpr int DPT_PER = 16;                        // pixels per thread: four float4 groups
constexpr int DPT_CH = DPT_THREADS * DPT_PER;      // pixels per workgroup
constexpr int DPT_MAX_ROWS_Y = 65535;

struct DptImg {
    const float *p;
    long long s0, s2, s3;
    int lin;                  // a frame's pixels are contiguous in raster order
};

struct DptArgs {
    int F, W, rows;           // rows: F (pred only: gt's statistics are given) or 2 F
    unsigned n;
    int nchunks;
    DptImg im[2];             // rows < F, rows >= F
    const float *gt_stats;    // [F, 2] or null
    unsigned *hist;           // [2F][4][256]
    unsigned *cnt;            // [2F][4]: NaNs, == t, > t, < t
    float *tval;              // [2F]
    double *part_abs;         // [2F][nchunks]
    double *part_d;           // [F][nchunks][3]
    float *lossf;             // [F]
    float gscale;
    float *grad;
    long long g0, g2, g3;
    int glin, accumulate;
    float *per_frame, *stats_out;
    int32_t *ties_out;
    float *stats;             // splat_depth_stats: [rows, 2]
};

// ordered key of a float: ascending as the values, -0 = +0
__device__ __forceinline__ unsigned dpt_key(float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float dpt_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ const float *dpt_row(const DptArgs &A, int row, int &which) {
    which = row >= A.F;
    const DptImg &im = A.im[which];
    return im.p + (long long)(which ? row - A.F : row) * im.s0;
}

// element offset of pixel i of a plane
__device__ __forceinline__ long long dpt_off(int lin, long long s2, long long s3, unsigned W, unsigned i) {
    if (lin) return (long long)i;
    const unsigned y = i / W, x = i - y * W;
    return (long long)y * s2 + (long long)x * s3;
}

// this thread's DPT_PER pixels of the chunk that starts at c0: v[4 k + j] = pixel c0 + (k * DPT_THREADS + tid) * 4 + j (where < n)
__device__ __forceinline__ unsigned dpt_idx(unsigned c0, int k, int tid) { return c0 + (unsigned)(k * DPT_THREADS + tid) * 4u; }

__device__ __forceinline__ void dpt_load(const float *base, const DptImg &im, unsigned W, unsigned c0, unsigned n, int tid,
                                         float (&v)[DPT_PER]) {
    const bool vec = im.lin && (((uintptr_t)base & 15) == 0);
#pragma unroll
    for (int k = 0; k < DPT_PER / 4; ++k) {
        const unsigned i = dpt_idx(c0, k, tid);
        if (vec && i < n && n - i >= 4u) {
            const float4 q = *(const float4 *)(base + i);
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // (i + j < n written without overflow: i may be within 4 of 2^32)
                const bool ok = i < n && (unsigned)j < n - i;
                v[4 * k + j] = ok ? base[dpt_off(im.lin, im.s2, im.s3, W, i + j)] : 0.f;
            }
        }
    }
}

__device__ __forceinline__ bool dpt_valid(unsigned c0, int k, int j, int tid, unsigned n) {
    const unsigned i = dpt_idx(c0, k, tid);
    return i < n && (unsigned)j < n - i;
}

// one wave: the bin of the 256 counters h that holds rank kk (0-based) and the count below that bin; the same in every lane
__device__ __forceinline__ void dpt_scan(const unsigned *h, unsigned kk, unsigned &bin, unsigned &below) {
    const int lane = threadIdx.x & (WAVE - 1);
    const uint4 q = *(const uint4 *)(h + 4 * lane);
    const unsigned s = (q.x + q.y) + (q.z + q.w);
    unsigned incl = s;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const unsigned excl = incl - s;
    unsigned b = 4 * lane, bl = excl;
    const bool hit = excl <= kk && kk < incl;
    if (hit) {
        if (bl + q.x <= kk) { bl += q.x; ++b;
            if (bl + q.y <= kk) { bl += q.y; ++b;
                if (bl + q.z <= kk) { bl += q.z; ++b; } } }
    }
    const unsigned long long m = __ballot(hit);
    const int src = m ? __ffsll((long long)m) - 1 : 0;      // (a row's counters always hold its rank; 0 keeps the reads in range)
    bin = __shfl(b, src);
    below = __shfl(bl, src);
    if (!m) { bin = 0; below = 0; }
}

// one wave: the key bits fixed by digits 0 .. D-1 of a row's select (every lane gets the same)
__device__ __forceinline__ unsigned dpt_prefix(const unsigned *hist_row, unsigned n, int D) {
    unsigned prefix = 0, kk = (n - 1u) / 2u;
    for (int d = 0; d < D; ++d) {
        unsigned bin, below;
        dpt_scan(hist_row + 256 * d, kk, bin, below);
        prefix |= bin << (24 - 8 * d);
        kk -= below;
    }
    return prefix;
}

// one wave: the chunk partials part[k * stride], k < nchunks, added in a fixed order (lane l takes k = l, l + 64, ...; then a
// butterfly, which gives every lane the same bits)
__device__ __forceinline__ double dpt_sum_partials(const double *part, int nchunks, int stride) {
    const int lane = threadIdx.x & (WAVE - 1);
    double s = 0.0;
    for (int k = lane; k < nchunks; k += WAVE) s += part[(long long)k * stride];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// workgroup sum of a double in a fixed order; the total in every thread
__device__ __forceinline__ double dpt_block_sum(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    const double t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}

template <int DIGIT>
__global__ void __launch_bounds__(DPT_THREADS) dpt_hist_kernel(DptArgs A) {
    __shared__ __attribute__((aligned(16))) unsigned hist[DPT_THREADS / WAVE][256];
    __shared__ unsigned sh_prefix;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const unsigned c0 = blockIdx.x * (unsigned)DPT_CH;
    constexpr unsigned pmask = DIGIT == 0 ? 0u : 0xffffffffu << (32 - 8 * DIGIT);
    constexpr int shift = 24 - 8 * DIGIT;
    for (int row = blockIdx.y; row < A.rows; row += gridDim.y) {
        int which;
        const float *base = dpt_row(A, row, which);
#pragma unroll
        for (int w = 0; w < DPT_THREADS / WAVE; ++w) hist[w][tid] = 0;
        if (DIGIT > 0 && wv == 0) {
            const unsigned p = dpt_prefix(A.hist + (long long)row * 1024, A.n, DIGIT);
            if (lane == 0) sh_prefix = p;
        }
        __syncthreads();
        const unsigned prefix = DIGIT > 0 ? sh_prefix : 0u;
        float v[DPT_PER];
        dpt_load(base, A.im[which], (unsigned)A.W, c0, A.n, tid, v);
        unsigned cur = 0, run = 0, nnan = 0;      // runs of one bin (a plateau) go to LDS as one add
#pragma unroll
        for (int e = 0; e < DPT_PER; ++e) {
            if (!dpt_valid(c0, e >> 2, e & 3, tid, A.n)) continue;
            const unsigned key = dpt_key(v[e]);
            if (DIGIT == 0) nnan += v[e] != v[e];
            if ((key & pmask) != prefix) continue;
            const unsigned b = (key >> shift) & 255u;
            if (run && b != cur) { atomicAdd(&hist[wv][cur], run); run = 0; }
            cur = b;
            ++run;
        }
        if (run) atomicAdd(&hist[wv][cur], run);
        __syncthreads();
        {
            const unsigned tot = (hist[0][tid] + hist[1][tid]) + (hist[2][tid] + hist[3][tid]);
            if (tot) atomicAdd(A.hist + (long long)row * 1024 + 256 * DIGIT + tid, tot);
        }
        if (DIGIT == 0) {
            nnan = wave_sum_u(nnan);
            if (lane == 0 && nnan) atomicAdd(A.cnt + 4ll * row, nnan);
        }
        __syncthreads();
    }
}

// launch 5: t of every row, the chunk's partial of sum |p - t|, the counts of p == t, p > t, p < t
__global__ void __launch_bounds__(DPT_THREADS) dpt_absdev_kernel(DptArgs A) {
    __shared__ unsigned sh_prefix;
    __shared__ double red[DPT_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const unsigned c0 = blockIdx.x * (unsigned)DPT_CH;
    for (int row = blockIdx.y; row < A.rows; row += gridDim.y) {
        int which;
        const float *base = dpt_row(A, row, which);
        if (wv == 0) {
            const unsigned p = dpt_prefix(A.hist + (long long)row * 1024, A.n, 4);
            if (lane == 0) sh_prefix = p;
        }
        __syncthreads();
        const float t = A.cnt[4ll * row] ? __builtin_nanf("") : dpt_unkey(sh_prefix);
        float v[DPT_PER];
        dpt_load(base, A.im[which], (unsigned)A.W, c0, A.n, tid, v);
        float acc = 0.f;
        unsigned eq = 0, gt = 0, lt = 0;
#pragma unroll
        for (int e = 0; e < DPT_PER; ++e) {
            if (!dpt_valid(c0, e >> 2, e & 3, tid, A.n)) continue;
            acc += fabsf(v[e] - t);
            eq += v[e] == t;
            gt += v[e] > t;
            lt += v[e] < t;
        }
        const double tot = dpt_block_sum((double)acc, red);
        eq = wave_sum_u(eq);
        gt = wave_sum_u(gt);
        lt = wave_sum_u(lt);
        if (lane == 0) {
            if (eq) atomicAdd(A.cnt + 4ll * row + 1, eq);
            if (gt) atomicAdd(A.cnt + 4ll * row + 2, gt);
            if (lt) atomicAdd(A.cnt + 4ll * row + 3, lt);
        }
        if (tid == 0) {
            A.part_abs[(long long)row * A.nchunks + blockIdx.x] = tot;
            if (blockIdx.x == 0) A.tval[row] = t;
        }
        __syncthreads();
    }
}

// s of a row from its chunk partials (one wave; the same bits wherever it is called)
__device__ __forceinline__ float dpt_scale_of(const DptArgs &A, int row) {
    return (float)(dpt_sum_partials(A.part_abs + (long long)row * A.nchunks, A.nchunks, 1) / (double)A.n);
}

// splat_depth_stats: (t, s) of every row
__global__ void __launch_bounds__(WAVE) dpt_stats_kernel(DptArgs A) {
    for (int row = blockIdx.x; row < A.rows; row += gridDim.x) {
        const float s = dpt_scale_of(A, row);
        if (threadIdx.x == 0) {
            A.stats[2ll * row] = A.tval[row];
            A.stats[2ll * row + 1] = s;
        }
    }
}

struct DptNorm {
    float tp, sp, tg, sg;
};

// one wave: the four statistics of frame f
__device__ __forceinline__ DptNorm dpt_norm(const DptArgs &A, int f) {
    DptNorm N;
    N.tp = A.tval[f];
    N.sp = dpt_scale_of(A, f);
    if (A.gt_stats) {
        N.tg = A.gt_stats[2ll * f];
        N.sg = A.gt_stats[2ll * f + 1];
    } else {
        N.tg = A.tval[A.F + f];
        N.sg = dpt_scale_of(A, A.F + f);
    }
    return N;
}

// launch 6: the chunk's partials of sum d^2, sum d, sum d (p - t_p)
__global__ void __launch_bounds__(DPT_THREADS) dpt_d_kernel(DptArgs A) {
    __shared__ DptNorm shN;
    __shared__ double red[DPT_THREADS / WAVE];
    const int tid = threadIdx.x, wv = tid / WAVE;
    const unsigned c0 = blockIdx.x * (unsigned)DPT_CH;
    for (int f = blockIdx.y; f < A.F; f += gridDim.y) {
        if (wv == 0) {
            const DptNorm N = dpt_norm(A, f);
            if (tid == 0) shN = N;
        }
        __syncthreads();
        const DptNorm N = shN;
        float p[DPT_PER], g[DPT_PER];
        dpt_load(A.im[0].p + (long long)f * A.im[0].s0, A.im[0], (unsigned)A.W, c0, A.n, tid, p);
        dpt_load(A.im[1].p + (long long)f * A.im[1].s0, A.im[1], (unsigned)A.W, c0, A.n, tid, g);
        float a2 = 0.f, a1 = 0.f, ab = 0.f;
#pragma unroll
        for (int e = 0; e < DPT_PER; ++e) {
            if (!dpt_valid(c0, e >> 2, e & 3, tid, A.n)) continue;
            const float dp = p[e] - N.tp;
            const float d = dp / N.sp - (g[e] - N.tg) / N.sg;
            a2 += d * d;
            a1 += d;
            ab += d * dp;
        }
        const double s2 = dpt_block_sum((double)a2, red);
        const double s1 = dpt_block_sum((double)a1, red);
        const double sb = dpt_block_sum((double)ab, red);
        if (tid == 0) {
            double *o = A.part_d + 3 * ((long long)f * A.nchunks + blockIdx.x);
            o[0] = s2; o[1] = s1; o[2] = sb;
        }
        __syncthreads();
    }
}

// launch 7: loss_f, A, B from the chunk partials; the frame's outputs (chunk 0); the gradient of the chunk's pixels (grad given)
__global__ void __launch_bounds__(DPT_THREADS) dpt_grad_kernel(DptArgs A) {
    __shared__ DptNorm shN;
    __shared__ float shc[3];          // 2 / n, B / (n s_p^2), the tie pixels' extra term
    const int tid = threadIdx.x, wv = tid / WAVE;
    const unsigned c0 = blockIdx.x * (unsigned)DPT_CH;
    for (int f = blockIdx.y; f < A.F; f += gridDim.y) {
        if (wv == 0) {
            const DptNorm N = dpt_norm(A, f);
            const double *pd = A.part_d + 3ll * f * A.nchunks;
            const double n = (double)A.n;
            const double sum2 = dpt_sum_partials(pd, A.nchunks, 3);
            const double Asum = 2.0 / n * dpt_sum_partials(pd + 1, A.nchunks, 3);
            const double Bsum = 2.0 / n * dpt_sum_partials(pd + 2, A.nchunks, 3);
            if (tid == 0) {
                const unsigned m = A.cnt[4ll * f + 1];
                const double S = (double)A.cnt[4ll * f + 2] - (double)A.cnt[4ll * f + 3];
                const double sp = (double)N.sp;
                const double c1 = Bsum / (n * sp * sp);
                shN = N;
                shc[0] = (float)(2.0 / n);
                shc[1] = (float)c1;
                shc[2] = (float)((-Asum / sp + c1 * S) / (double)m);
                if (blockIdx.x == 0) {
                    const float loss = (float)(sum2 / n);
                    A.lossf[f] = loss;
                    if (A.per_frame) A.per_frame[f] = loss;
                    if (A.stats_out) {
                        float *o = A.stats_out + 4ll * f;
                        o[0] = N.tp; o[1] = N.sp; o[2] = N.tg; o[3] = N.sg;
                    }
                    if (A.ties_out) A.ties_out[f] = (int32_t)m;
                }
            }
        }
        __syncthreads();
        if (A.grad) {
            const DptNorm N = shN;
            const float c2n = shc[0], c1 = shc[1], tie = shc[2], gs = A.gscale;
            float p[DPT_PER], g[DPT_PER];
            dpt_load(A.im[0].p + (long long)f * A.im[0].s0, A.im[0], (unsigned)A.W, c0, A.n, tid, p);
            dpt_load(A.im[1].p + (long long)f * A.im[1].s0, A.im[1], (unsigned)A.W, c0, A.n, tid, g);
            float *gb = A.grad + (long long)f * A.g0;
            const bool vec = A.glin && (((uintptr_t)gb & 15) == 0);
#pragma unroll
            for (int k = 0; k < DPT_PER / 4; ++k) {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float pe = p[4 * k + j];
                    const float dp = pe - N.tp;
                    const float d = dp / N.sp - (g[4 * k + j] - N.tg) / N.sg;
                    float r = (d * c2n) / N.sp;
                    r -= pe > N.tp ? c1 : (pe < N.tp ? -c1 : 0.f);
                    if (pe == N.tp) r += tie;
                    o[j] = gs * r;
                }
                const unsigned i = dpt_idx(c0, k, tid);
                if (vec && i < A.n && A.n - i >= 4u) {
                    float4 *dst = (float4 *)(gb + i);
                    float4 q = make_float4(o[0], o[1], o[2], o[3]);
                    if (A.accumulate) {
                        const float4 old = *dst;
                        q.x += old.x; q.y += old.y; q.z += old.z; q.w += old.w;
                    }
                    *dst = q;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (!dpt_valid(c0, k, j, tid, A.n)) continue;
                        float *dst = gb + dpt_off(A.glin, A.g2, A.g3, (unsigned)A.W, i + j);
                        *dst = A.accumulate ? *dst + o[j] : o[j];
                    }
                }
            }
        }
        __syncthreads();
    }
}

int dpt_lin(int H, int W, const int64_t *s) { return (W == 1 || s[3] == 1) && (H == 1 || s[2] == W); }

size_t dpt_align(size_t b) { return (b + 255) & ~(size_t)255; }

bool dpt_sizes_ok(int F, int H, int W) {
    return F >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL && F <= (1 << 24);
}

// scratch: [hist | cnt] (zeroed together), tval, part_abs, part_d, lossf -- always sized for 2 F rows
struct DptScratch {
    size_t hist, cnt, zero_bytes, tval, part_abs, part_d, lossf, total;
    int nchunks;
};

DptScratch dpt_scratch(int F, int H, int W) {
    DptScratch S;
    const size_t R = 2 * (size_t)F, n = (size_t)H * W;
    S.nchunks = (int)((n + DPT_CH - 1) / DPT_CH);
    size_t o = 0;
    S.hist = o; o += R * 1024 * sizeof(unsigned);
    S.cnt = o; o += R * 4 * sizeof(unsigned);
    S.zero_bytes = o;
    o = dpt_align(o);
    S.tval = o; o = dpt_align(o + R * sizeof(float));
    S.part_abs = o; o = dpt_align(o + R * S.nchunks * sizeof(double));
    S.part_d = o; o = dpt_align(o + (size_t)F * S.nchunks * 3 * sizeof(double));
    S.lossf = o; o = dpt_align(o + (size_t)F * sizeof(float));
    S.total = o;
    return S;
}

void dpt_bind(DptArgs &A, const DptScratch &S, void *scratch) {
    char *b = (char *)scratch;
    A.hist = (unsigned *)(b + S.hist);
    A.cnt = (unsigned *)(b + S.cnt);
    A.tval = (float *)(b + S.tval);
    A.part_abs = (double *)(b + S.part_abs);
    A.part_d = (double *)(b + S.part_d);
    A.lossf = (float *)(b + S.lossf);
    A.nchunks = S.nchunks;
}

DptImg dpt_img(int H, int W, const float *p, const int64_t *s) {
    DptImg I;
    I.p = p; I.s0 = s[0]; I.s2 = s[2]; I.s3 = s[3];
    I.lin = dpt_lin(H, W, s);
    return I;
}

// launches 0 - 5 on A.rows rows
int dpt_select_rows(const DptArgs &A, const DptScratch &S, void *scratch, hipStream_t s) {
    SPLAT_CHECK_HIP(hipMemsetAsync(scratch, 0, S.zero_bytes, s));
    const dim3 grid((unsigned)A.nchunks, (unsigned)std::min(A.rows, DPT_MAX_ROWS_Y)), block(DPT_THREADS);
    SPLAT_LAUNCH("depth_dpt_hist", dpt_hist_kernel<0>, grid, block, 0, s, A);
    SPLAT_LAUNCH("depth_dpt_hist", dpt_hist_kernel<1>, grid, block, 0, s, A);
    SPLAT_LAUNCH("depth_dpt_hist", dpt_hist_kernel<2>, grid, block, 0, s, A);
    SPLAT_LAUNCH("depth_dpt_hist", dpt_hist_kernel<3>, grid, block, 0, s, A);
    SPLAT_LAUNCH("depth_dpt_absdev", dpt_absdev_kernel, grid, block, 0, s, A);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

}  // namespace

extern "C" size_t splat_depth_dpt_scratch_bytes(int F, int H, int W) {
    if (!dpt_sizes_ok(F, H, W)) return 0;
    return dpt_scratch(F, H, W).total;
}

extern "C" int splat_depth_stats(int F, int H, int W, const float *img, const int64_t *strides, float *stats, void *scratch,
                                 splat_stream_t stream) {
    SPLAT_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "bad sizes (F, H, W >= 1)");
    SPLAT_CHECK_ARG(dpt_sizes_ok(F, H, W), "sizes too large (H W <= 2^31 - 1, F <= 2^24)");
    SPLAT_CHECK_ARG(img && strides && stats && scratch, "null pointer");
    for (int k = 0; k < 4; ++k) SPLAT_CHECK_ARG(strides[k] >= 0, "strides must be >= 0");
    const hipStream_t s = (hipStream_t)stream;
    const DptScratch S = dpt_scratch(F, H, W);
    DptArgs A;
    memset(&A, 0, sizeof(A));
    A.F = F; A.W = W; A.rows = F; A.n = (unsigned)((long long)H * W);
    A.im[0] = A.im[1] = dpt_img(H, W, img, strides);
    A.stats = stats;
    dpt_bind(A, S, scratch);
    const int rc = dpt_select_rows(A, S, scratch, s);
    if (rc) return rc;
    SPLAT_LAUNCH("depth_dpt_stats", dpt_stats_kernel, dim3((unsigned)std::min(F, DPT_MAX_ROWS_Y)), dim3(WAVE), 0, s, A);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_depth_dpt_loss_grad(int F, int H, int W, const float *pred, const int64_t *pred_strides, const float *gt,
                                         const int64_t *gt_strides, const float *gt_stats, float scale, float *grad,
                                         const int64_t *grad_strides, int accumulate, float *per_frame, float *loss_slot,
                                         float *stats_out, int32_t *ties_out, void *scratch, splat_stream_t stream) {
    SPLAT_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "bad sizes (F, H, W >= 1)");
    SPLAT_CHECK_ARG(dpt_sizes_ok(F, H, W), "sizes too large (H W <= 2^31 - 1, F <= 2^24)");
    SPLAT_CHECK_ARG(pred && pred_strides && gt && gt_strides && scratch, "null pointer");
    for (int k = 0; k < 4; ++k) SPLAT_CHECK_ARG(pred_strides[k] >= 0 && gt_strides[k] >= 0, "strides must be >= 0");
    if (grad) {
        SPLAT_CHECK_ARG(grad_strides, "null pointer (grad_strides)");
        for (int k = 0; k < 4; ++k) SPLAT_CHECK_ARG(grad_strides[k] >= 0, "strides must be >= 0");
    }
    const hipStream_t s = (hipStream_t)stream;
    const DptScratch S = dpt_scratch(F, H, W);
    DptArgs A;
    memset(&A, 0, sizeof(A));
    A.F = F; A.W = W; A.rows = gt_stats ? F : 2 * F; A.n = (unsigned)((long long)H * W);
    A.im[0] = dpt_img(H, W, pred, pred_strides);
    A.im[1] = dpt_img(H, W, gt, gt_strides);
    A.gt_stats = gt_stats;
    A.gscale = scale / (float)F;
    A.grad = grad;
    if (grad) {
        A.g0 = grad_strides[0]; A.g2 = grad_strides[2]; A.g3 = grad_strides[3];
        A.glin = dpt_lin(H, W, grad_strides);
    }
    A.accumulate = accumulate ? 1 : 0;
    A.per_frame = per_frame; A.stats_out = stats_out; A.ties_out = ties_out;
    dpt_bind(A, S, scratch);
    const int rc = dpt_select_rows(A, S, scratch, s);
    if (rc) return rc;
    const unsigned gy = (unsigned)std::min(F, DPT_MAX_ROWS_Y);
    SPLAT_LAUNCH("depth_dpt_d", dpt_d_kernel, dim3((unsigned)A.nchunks, gy), dim3(DPT_THREADS), 0, s, A);
    // without a gradient image only the frames' outputs are left: one workgroup per frame
    SPLAT_LAUNCH("depth_dpt_grad", dpt_grad_kernel, dim3(grad ? (unsigned)A.nchunks : 1u, gy), dim3(DPT_THREADS), 0, s, A);
    SPLAT_POST_LAUNCH();
    if (loss_slot) {
        SPLAT_LAUNCH("depth_dpt_slot", track_loss_slot_kernel, dim3(1), dim3(WAVE), 0, s, F, (const float *)A.lossf, loss_slot);
        SPLAT_POST_LAUNCH();
    }
    return SPLAT_OK;
}
