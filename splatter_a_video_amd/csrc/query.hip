// Point tracking: compositing at sparse sub-pixel query points, and the feature rows of a tracking query.
// Reference semantics: F.grid_sample(alpha_blending(...)[None], grid, mode="bilinear", padding_mode="zeros",
// align_corners=True) as draw_pixel_trajectory and get_correspondences_and_occlusion_masks_for_pixels_core use it
// (src/trainer_fragGS.py:1483-1566, :1644-1677) -- without the dense image: only the four bilinear corner pixels of every
// query walk their tile lists.
//
// MI355X design:
//   * one 256-thread workgroup per query = four waves, wave w = corner w (nw, ne, sw, se).  A corner outside the image
//     walks nothing.
//   * the alpha of a list entry does not depend on the transmittance: 64 entries are evaluated at once, lane = entry
//     (gather of uv / conic / opacity by id, power_coeffs + power_poly + exp2_guard of blend_power.h: the forward's bits).
//   * the transmittance chain T <- T (1 - alpha) is the forward's, in list order, over the entries that passed alpha >= 1/255
//     only (ballot), on wave-uniform values read out of the lanes; an applied entry leaves its weight alpha T in its lane.
//   * then lanes are CHANNELS: the applied entries' feature rows are read one coalesced row per entry (four rows in flight)
//     and accumulated F[c] += f[id, c] w in list order, ceil(cn / 64) <= NA accumulators per lane; rows wider than 64 NA
//     channels take one launch per chunk.
//   * the four corner values (F + T bg) meet in LDS and are combined nw, ne, sw, se with the bilinear weights.  No
//     atomics anywhere in the forward: results are bit-reproducible.
//   * every kernel takes its corner from points_corner and a list entry's alpha from points_entry: the forward and the
//     backward's replay decide with the same bits because they run the same code; the backward kernels take the six geometry
//     terms from points_geo_terms.
//   * the backward replays every corner's list back to front: points_bwd_kernel adds with float atomics (per-Gaussian buffers,
//     or the frame batch's pair records in its BATCH instantiation), points_bwd_ordered_kernel with plain load / add / store
//     into slot records that one wave owns.  The two replay loops are still written out twice: hipcc picks which product of
//     acc = a f + (1 - a) acc it fuses per loop shape, so a shared loop changes the gradient's bits.
//   * the frame-batched entries (BATCH instantiations of the forward and the atomic backward) take the queries of F frames in
//     CSR form: the frame of a query comes from `offsets` on the device (F is a few dozen: a scalar scan) and the FrameBatch
//     buffers are read through their frame strides.
#include <type_traits>

#include "blend_power.h"
#include "dynamics_dev.h"
#include "pointwise_dev.h"

namespace {

constexpr int PT_NA_MAX = 4;                  // accumulators per lane: channel chunks of at most 256
constexpr int PT_CHUNK = 64 * PT_NA_MAX;

// what the forward and the backward kernels both read
struct PointsGeo {
    int P, C, c0, cn;
    const float2 *uv;
    const float *conic, *opacity, *feature;
    const int *idx_sorted;
    const int2 *tile_range;
    float bg;
    int W, H, gx;
    const float2 *points;
};

struct PointsArgs : PointsGeo {
    float *out;       // [Q, C]
    float *corner_T;  // [Q, 4] or NULL
    int *corner_n;    // [Q, 4] or NULL
};

struct PointsBwdArgs : PointsGeo {
    const float *corner_T;   // [Q, 4]
    const int *corner_n;     // [Q, 4]
    const float *dL_dout;    // [Q, C]
    float *dL_duv, *dL_dconic, *dL_dopacity, *dL_dfeature;   // each may be NULL
};

__device__ __forceinline__ float lane_f(float v, int j) {
    return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(v), j));
}

// The frame-batched view (BATCH kernels): the queries offsets[f] .. offsets[f + 1] belong to frame f, whose buffers lie
// f * stride behind the batch's base pointers (uv [F,P,2], conic [F,P,3], idx_sorted / slot_sorted [F,cap], tile_range [F,T,2];
// opacity, feature and dL_dfeature with their own frame strides, 0 = shared by the frames).
struct PointsBatch {
    int F, T;
    const long long *offsets;   // device int64 [F + 1]
    long long Q, cap, opacity_fs, feature_fs, dfeature_fs;
    // backward: the geometry gradients go into the pair records of the frame batch (record of frame f, slot s at
    // rec + (f * cap + s) * rec_stride floats; fields REC_UX .. REC_O of common.h)
    const int *slot_sorted;
    float *rec;
    int rec_stride, detach_opacity;
};

// frame of query q: the first f with 0 <= offsets[f] <= q < offsets[f + 1] <= Q, or -1 (malformed offsets: nobody owns q).
// Uniform per workgroup: scalar loads.
__device__ __forceinline__ int points_frame_of(const PointsBatch &B, long long q) {
    int f = -1;
    for (int i = B.F - 1; i >= 0; --i) {
        const long long o0 = B.offsets[i], o1 = B.offsets[i + 1];
        if (0 <= o0 && o0 <= q && q < o1 && o1 <= B.Q) f = i;
    }
    return f;
}

__device__ __forceinline__ void points_frame_view(PointsGeo &A, const PointsBatch &B, int f) {
    const size_t fz = (size_t)f;
    A.uv += fz * (size_t)A.P;
    A.conic += fz * 3 * (size_t)A.P;
    A.opacity += fz * (size_t)B.opacity_fs;
    A.feature += fz * (size_t)B.feature_fs;
    if (A.idx_sorted) A.idx_sorted += fz * (size_t)B.cap;
    A.tile_range += fz * (size_t)B.T;
}

// Corner k (nw, ne, sw, se) of the query at pt.  `in`: the in / out test in float, before any conversion to int (1e9, inf and
// NaN are simply outside); cw: its bilinear weight (pt is finite where `in` holds).  Where `in` holds: the corner's pixel and
// tile, the pixel relative to the tile centre with its monomials (exact in f32), and the tile centre as the dense forward forms it.
struct PointsCorner {
    bool in;
    float cw;
    int px, py, tx, ty;
    float x, y, xx, xy, yy, tcx, tcy;
};

__device__ __forceinline__ PointsCorner points_corner(float2 pt, int k, int W, int H) {
    PointsCorner K;
    const float x0f = floorf(pt.x), y0f = floorf(pt.y);
    const float cxf = x0f + (float)(k & 1), cyf = y0f + (float)(k >> 1);
    K.in = cxf >= 0.f && cxf <= (float)(W - 1) && cyf >= 0.f && cyf <= (float)(H - 1);
    K.cw = ((k & 1) ? pt.x - x0f : (x0f + 1.f) - pt.x) * ((k >> 1) ? pt.y - y0f : (y0f + 1.f) - pt.y);
    K.px = (int)cxf; K.py = (int)cyf;
    K.tx = K.px / TILE; K.ty = K.py / TILE;
    K.x = (float)(K.px - K.tx * TILE) - 7.5f; K.y = (float)(K.py - K.ty * TILE) - 7.5f;
    K.xx = K.x * K.x; K.xy = K.x * K.y; K.yy = K.y * K.y;
    K.tcx = (float)(K.tx * TILE) + 7.5f; K.tcy = (float)(K.ty * TILE) + 7.5f;
    return K;
}

// lane = entry: entry e of the list that starts at idx_sorted[first] (n entries count) on corner K -- its alpha with the dense
// forward's arithmetic, and what the backward needs besides: the unclamped araw and the gathered operands.
struct PointsEntry {
    int id;        // -1 unless e < n and the id lies inside the set (an id outside is skipped, never dereferenced)
    int slot;      // slots[first + e] of such an entry where the caller passes `slots` (issued with the gathers), else -1
    float alpha, araw, ux, uy, cA, cB, cC, o;
};

__device__ __forceinline__ bool points_entry(const PointsGeo &A, const PointsCorner &K, int first, int e, int n, PointsEntry &E,
                                             const int *slots = nullptr) {
    bool aok = false;
    E = {-1, -1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    if (e < n) {
        const int id = A.idx_sorted[first + e];
        if ((unsigned)id < (unsigned)A.P) {
            E.id = id;
            const float2 c = A.uv[id];
            E.ux = c.x; E.uy = c.y;
            E.cA = A.conic[3 * (size_t)id]; E.cB = A.conic[3 * (size_t)id + 1]; E.cC = A.conic[3 * (size_t)id + 2];
            E.o = A.opacity[id];
            if (slots) E.slot = slots[first + e];
            const PowerCoef k = power_coeffs(E.ux, E.uy, E.cA, E.cB, E.cC, E.o, K.tcx, K.tcy);
            const float pw = power_poly(make_float4(k.q0, k.qx, k.qy, k.qxx), make_float4(k.qxy, k.qyy, 0.f, 0.f), K.x, K.y, K.xx, K.xy, K.yy);
            bool pw_ok;
            E.araw = exp2_guard(pw, pw_ok);
            const float a = fminf(0.99f, E.araw);
            aok = pw_ok && !(a < (1.0f / 255.0f));
            E.alpha = aok ? a : 0.f;
        }
    }
    return aok;
}

// The six geometry terms of an applied entry on the corner pixel (pxf, pyf), dLa = its dL_dalpha (replay_one's expressions), as
// products a[i] * b[i] for the fields i = REC_UX .. REC_O.  The ONE copy: the backward kernels only add.  A caller forms the
// product where it adds, so that an atomic adds the rounded product and a load / add / store may fuse it, as they always did.
struct PointsGeoTerms {
    float a[REC_GEOM], b[REC_GEOM];
};

__device__ __forceinline__ PointsGeoTerms points_geo_terms(const PointsEntry &E, float pxf, float pyf, float dLa) {
    const float dx = E.ux - pxf, dy = E.uy - pyf;
    const float G = E.araw * __builtin_amdgcn_rcpf(E.o);
    const float dLG = E.o * dLa;
    PointsGeoTerms t;
    t.a[REC_UX] = dLG; t.b[REC_UX] = -G * dx * E.cA - G * dy * E.cB;
    t.a[REC_UY] = dLG; t.b[REC_UY] = -G * dy * E.cC - G * dx * E.cB;
    t.a[REC_CA] = -0.5f * G * dx * dx; t.b[REC_CA] = dLG;
    t.a[REC_CB] = -G * dx * dy; t.b[REC_CB] = dLG;
    t.a[REC_CC] = -0.5f * G * dy * dy; t.b[REC_CC] = dLG;
    t.a[REC_O] = G; t.b[REC_O] = dLa;
    return t;
}

// LIVE: an in-image corner whose bilinear weight is zero is not walked either (it reports T = 0, ncontrib = 0 like a corner
// outside and adds 0 * bg = 0: the same value bits for finite features) -- the differentiable route's forward, whose backward
// replays only the corners that carry weight; an integer query pixel then walks one list instead of four.
template <int NA, bool LIVE, bool BATCH>
__global__ void __launch_bounds__(256) points_fwd_kernel(const PointsArgs A0, const PointsBatch B) {
    __shared__ float s_val[4][64 * NA];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave = corner: uniform, so the walk below branches on scalars
    const size_t q = blockIdx.x;
    PointsArgs A = A0;
    if (BATCH) {
        const int f = points_frame_of(B, (long long)q);
        if (f < 0) {   // a query no frame owns: a row of zeros, nothing dereferenced (uniform: the whole workgroup leaves)
            for (int c = tid; c < A.cn; c += 256) A.out[q * (size_t)A.C + A.c0 + c] = 0.f;
            if (tid < 4) {
                if (A.corner_T) A.corner_T[q * 4 + tid] = 0.f;
                if (A.corner_n) A.corner_n[q * 4 + tid] = 0;
            }
            return;
        }
        if (A.P > 0) points_frame_view(A, B, f);
    }
    const float2 pt = A.points[q];
    const PointsCorner K = points_corner(pt, w, A.W, A.H);
    const bool in = K.in && (!LIVE || K.cw != 0.f);

    float T = 1.f;
    int last = 0;
    float F[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) F[k] = 0.f;

    if (in) {
        int2 range = make_int2(0, 0);
        if (A.P > 0) range = A.tile_range[K.ty * A.gx + K.tx];
        const int n = imax_(range.y - range.x, 0);
        bool done = false;
        for (int base = 0; base < n && !done; base += WAVE) {
            // ---- lane = entry: its alpha on this pixel
            PointsEntry E;
            const bool aok = points_entry(A, K, range.x, base + lane, n, E);
            // ---- the transmittance chain over the entries that touch the pixel, in list order (wave-uniform values)
            unsigned long long cand = __ballot(aok), applied = 0ull;
            float wv = 0.f;   // lane j: weight alpha T of entry base + j, if it applied
            while (cand) {
                const int j = (int)__builtin_ctzll(cand);
                cand &= cand - 1ull;
                const float a = lane_f(E.alpha, j);
                const float nT = T * (1.f - a);
                if (nT < 0.0001f) {   // the splat that would take T below 1e-4 ends the pixel, unapplied
                    done = true;
                    break;
                }
                const float wgt = a * T;
                wv = lane == j ? wgt : wv;
                T = nT;
                last = base + j + 1;
                applied |= 1ull << j;
            }
            // ---- lane = channel: the applied entries' rows, four in flight, accumulated in list order
            const float *fbase = A.feature + A.c0 + lane;
            while (__popcll(applied) >= 4) {
                int jj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    jj[u] = (int)__builtin_ctzll(applied);
                    applied &= applied - 1ull;
                }
                float f[4][NA], wg[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float *row = fbase + (size_t)__builtin_amdgcn_readlane(E.id, jj[u]) * (size_t)A.C;
                    wg[u] = lane_f(wv, jj[u]);
#pragma unroll
                    for (int k = 0; k < NA; ++k) f[u][k] = (lane + 64 * k < A.cn) ? row[64 * k] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int k = 0; k < NA; ++k) F[k] = __builtin_fmaf(f[u][k], wg[u], F[k]);
            }
            while (applied) {
                const int j = (int)__builtin_ctzll(applied);
                applied &= applied - 1ull;
                const float *row = fbase + (size_t)__builtin_amdgcn_readlane(E.id, j) * (size_t)A.C;
                const float wg = lane_f(wv, j);
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    const float f = (lane + 64 * k < A.cn) ? row[64 * k] : 0.f;
                    F[k] = __builtin_fmaf(f, wg, F[k]);
                }
            }
        }
        if (lane == 0) {
            if (A.corner_T) A.corner_T[q * 4 + w] = T;
            if (A.corner_n) A.corner_n[q * 4 + w] = last;
        }
    } else if (lane == 0) {
        if (A.corner_T) A.corner_T[q * 4 + w] = 0.f;
        if (A.corner_n) A.corner_n[q * 4 + w] = 0;
    }
    // ---- the four corners meet: value = F + T bg, combined nw, ne, sw, se with the bilinear weights
#pragma unroll
    for (int k = 0; k < NA; ++k) s_val[w][64 * k + lane] = F[k] + T * A.bg;
    __syncthreads();
    bool cin[4];
    float cw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const PointsCorner Kk = points_corner(pt, k, A.W, A.H);
        cin[k] = Kk.in;
        cw[k] = Kk.cw;
    }
    for (int c = tid; c < A.cn; c += 256) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cin[k]) acc += s_val[k][c] * cw[k];   // a corner outside the image contributes nothing
        A.out[q * (size_t)A.C + A.c0 + c] = acc;
    }
}

// ---- host side: what the entries below share
// SPLAT_CHECK_ARG inside a helper: the message names the entry `fn`
#define PT_CHECK(fn, cond, msg)                    \
    do {                                           \
        if (!(cond)) {                             \
            splat_set_error("%s: %s", fn, msg);    \
            return SPLAT_E_ARG;                    \
        }                                          \
    } while (0)

long long points_num_tiles(int W, int H) { return (long long)((W + TILE - 1) / TILE) * (long long)((H + TILE - 1) / TILE); }

template <typename Args>
Args points_args(int P, int C, const float *uv, const float *conic, const float *opacity, const float *feature,
                 const int32_t *idx_sorted, const int32_t *tile_range, float bg, int W, int H, const float *points) {
    Args A;
    memset(&A, 0, sizeof(A));
    A.P = P; A.C = C;
    A.uv = (const float2 *)uv; A.conic = conic; A.opacity = opacity; A.feature = feature;
    A.idx_sorted = idx_sorted; A.tile_range = (const int2 *)tile_range;
    A.bg = bg; A.W = W; A.H = H; A.gx = (W + TILE - 1) / TILE;
    A.points = (const float2 *)points;
    return A;
}

PointsBatch points_batch(int F, int W, int H, const int64_t *offsets, int64_t Q, int64_t capacity, int64_t opacity_fs,
                         int64_t feature_fs) {
    PointsBatch B;
    memset(&B, 0, sizeof(B));
    B.F = F; B.T = (int)points_num_tiles(W, H);
    B.offsets = (const long long *)offsets; B.Q = Q; B.cap = capacity;
    B.opacity_fs = opacity_fs; B.feature_fs = feature_fs;
    return B;
}

// One launch per 256 channels: launch(A, std::integral_constant<int, NA>) starts the NA = ceil(cn / 64) instantiation of a kernel
// family on the chunk A.c0 .. A.c0 + A.cn.  Launches on one stream: the chunks run in ascending order.
template <typename Args, typename Launch>
int points_chunks(Args A, Launch launch) {
    for (int c0 = 0; c0 < A.C; c0 += PT_CHUNK) {
        A.c0 = c0;
        A.cn = A.C - c0 > PT_CHUNK ? PT_CHUNK : A.C - c0;
        switch ((A.cn + 63) / 64) {
            case 1: launch(A, std::integral_constant<int, 1>()); break;
            case 2: launch(A, std::integral_constant<int, 2>()); break;
            case 3: launch(A, std::integral_constant<int, 3>()); break;
            default: launch(A, std::integral_constant<int, 4>()); break;
        }
        SPLAT_POST_LAUNCH();
    }
    return SPLAT_OK;
}

// the launches of the validated forward
int points_forward(const PointsArgs &A0, int Q, bool live, hipStream_t s, const PointsBatch *batch = nullptr) {
    const PointsBatch B = batch ? *batch : points_batch(0, 0, 0, nullptr, 0, 0, 0, 0);
    return points_chunks(A0, [&](PointsArgs A, auto na) {
        constexpr int NA = decltype(na)::value;
        if (A.c0 != 0) {   // every chunk walks the same lists: the first one reports them
            A.corner_T = nullptr;
            A.corner_n = nullptr;
        }
        if (batch) SPLAT_LAUNCH("blend_points", (points_fwd_kernel<NA, true, true>), dim3((unsigned)Q), dim3(256), 0, s, A, B);
        else if (live) SPLAT_LAUNCH("blend_points", (points_fwd_kernel<NA, true, false>), dim3((unsigned)Q), dim3(256), 0, s, A, B);
        else SPLAT_LAUNCH("blend_points", (points_fwd_kernel<NA, false, false>), dim3((unsigned)Q), dim3(256), 0, s, A, B);
    });
}

int points_forward_entry(const char *fn, bool live, int P, int C, const float *uv, const float *conic, const float *opacity,
                         const float *feature, const int32_t *idx_sorted, const int32_t *tile_range, float bg, int W, int H, int Q,
                         const float *points, float *out, float *corner_T, int32_t *corner_ncontrib, splat_stream_t stream) {
    PT_CHECK(fn, P >= 0 && C >= 1 && W > 0 && H > 0 && Q >= 0, "bad sizes (P, Q >= 0, C, W, H >= 1)");
    PT_CHECK(fn, W <= (1 << 24) && H <= (1 << 24), "sizes too large (W, H <= 2^24: pixel indices are compared in float32)");
    if (Q == 0) return SPLAT_OK;
    PT_CHECK(fn, points && out, "null pointer (points / out)");
    // idx_sorted may be NULL when no Gaussian touches any tile (every tile range is empty, nothing dereferences it)
    PT_CHECK(fn, P == 0 || (uv && conic && opacity && feature && tile_range), "null pointer");
    PointsArgs A = points_args<PointsArgs>(P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, points);
    A.out = out; A.corner_T = corner_T; A.corner_n = corner_ncontrib;
    return points_forward(A, Q, live, (hipStream_t)stream);
}

// ---- backward of the sparse compositing: the gradient of grid_sample(alpha_blending(...)) w.r.t. uv, conic, opacity, feature.
// Corner pixel k of query q receives dL_dpix[c] = w_k(q) dL_dout[q, c] and replays its list back to front from the forward's
// corner_T / corner_ncontrib (the dense backward's per-pixel replay, replay_one of blend.hip: T by division, the bg term, the
// 0.99 clamp not masked).  Wave = corner as in the forward; a corner outside the image or with zero weight exits at once.
//   * lane = entry: 64 entries' alphas at once with the forward's arithmetic; applied = position < ncontrib and alpha >= 1/255.
//   * lane = channel: the applied entries back to front, four feature rows in flight; acc_c and g_c in registers, the dot
//     sum_c (f_c - acc_c) g_c by one DPP wave reduction, alpha T g_c added to dL_dfeature[id, c] with one coalesced row of float
//     atomics; the entry's dL_dalpha stays in the entry's lane.
//   * lane = entry again: the uv / conic / opacity atomics of the block issue from up to 64 lanes at once.
// Many queries hit one Gaussian: float atomics, outputs ADDED (the host entry refuses deterministic mode).
// BATCH: the queries of F frames (PointsBatch).  The geometry gradients of an applied entry at list position e of frame f are
// added to the pair record at slot slot_sorted[f, range.x + e] of that frame -- the record the tile backward of the same forward
// wrote for this (Gaussian, tile) pair, which the Gaussian-side walk sums per Gaussian afterwards.
template <int NA, bool BATCH>
__global__ void __launch_bounds__(256) points_bwd_kernel(const PointsBwdArgs A0, const PointsBatch B) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave = corner
    const size_t q = blockIdx.x;
    PointsBwdArgs A = A0;
    const int *slots = nullptr;   // BATCH: the frame's slot_sorted
    float *recs = nullptr;        //        and its pair records
    if (BATCH) {
        const int f = points_frame_of(B, (long long)q);
        if (f < 0) return;        // a query no frame owns
        points_frame_view(A, B, f);
        if (A.dL_dfeature) A.dL_dfeature += (size_t)f * (size_t)B.dfeature_fs;
        if (B.rec) {
            slots = B.slot_sorted + (size_t)f * (size_t)B.cap;
            recs = B.rec + (size_t)f * (size_t)B.cap * (size_t)B.rec_stride;
        }
    }
    const float2 ptv = A.points[q];
    // (uniform: the exits below are scalar branches)
    const PointsCorner K = points_corner(make_float2(lane_f(ptv.x, 0), lane_f(ptv.y, 0)), w, A.W, A.H);
    if (!K.in) return;
    const float cw = K.cw;
    if (cw == 0.f) return;
    const int2 range = A.tile_range[K.ty * A.gx + K.tx];
    const int n = imax_(range.y - range.x, 0);
    const int last = imin_(__builtin_amdgcn_readfirstlane(A.corner_n[q * 4 + w]), n);   // (never past the list)
    if (last <= 0) return;   // nothing applied: no Gaussian saw this corner
    const float Tf = lane_f(A.corner_T[q * 4 + w], 0);
    const float pxf = (float)K.px, pyf = (float)K.py;

    float g[NA], acc[NA];
    float gsum = 0.f;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        g[k] = (lane + 64 * k < A.cn) ? cw * A.dL_dout[q * (size_t)A.C + A.c0 + lane + 64 * k] : 0.f;
        acc[k] = 0.f;
        gsum += g[k];
    }
    const float bgdot = A.bg * wave_sum_bcast(gsum);
    float T = Tf;
    const float *fbase = A.feature + A.c0 + lane;
    float *dfbase = A.dL_dfeature ? A.dL_dfeature + A.c0 + lane : nullptr;

    for (int base = ((last - 1) / WAVE) * WAVE; base >= 0; base -= WAVE) {
        // ---- lane = entry: its alpha on this pixel (the forward's bits)
        const int e = base + lane;
        PointsEntry E;
        const bool aok = points_entry(A, K, range.x, e, last, E);
        const int id = E.id;
        const float alpha = E.alpha;
        // ---- lane = channel: the applied entries back to front, four rows in flight
        unsigned long long ap = __ballot(aok);
        float dLa_v = 0.f;   // lane j: dL_dalpha of entry base + j, if it applied
        while (ap) {
            int jj[4];
            float f[4][NA];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                jj[u] = ap ? 63 - (int)__builtin_clzll(ap) : -1;
                if (jj[u] >= 0) {
                    ap &= ~(1ull << jj[u]);
                    const float *row = fbase + (size_t)__builtin_amdgcn_readlane(id, jj[u]) * (size_t)A.C;
#pragma unroll
                    for (int k = 0; k < NA; ++k) f[u][k] = (lane + 64 * k < A.cn) ? row[64 * k] : 0.f;
                } else {
#pragma unroll
                    for (int k = 0; k < NA; ++k) f[u][k] = 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (jj[u] < 0) break;
                const int j = jj[u];
                const float a = lane_f(alpha, j);
                const float r1a = __builtin_amdgcn_rcpf(1.f - a);
                T = T * r1a;   // the transmittance in front of the entry
                const float wgt = a * T;
                float part = 0.f;
#pragma unroll
                for (int k = 0; k < NA; ++k) part += (f[u][k] - acc[k]) * g[k];
                float dLa = wave_sum_bcast(part) * T;
                dLa += (-Tf * r1a) * bgdot;
                dLa_v = lane == j ? dLa : dLa_v;
                if (dfbase) {
                    float *drow = dfbase + (size_t)__builtin_amdgcn_readlane(id, j) * (size_t)A.C;
#pragma unroll
                    for (int k = 0; k < NA; ++k)
                        if (lane + 64 * k < A.cn) atomic_add_f32(drow + 64 * k, wgt * g[k]);
                }
#pragma unroll
                for (int k = 0; k < NA; ++k) acc[k] = a * f[u][k] + (1.f - a) * acc[k];
            }
        }
        // ---- lane = entry: the geometry gradients of the block's applied entries (replay_one's expressions)
        if (aok) {
            const PointsGeoTerms t = points_geo_terms(E, pxf, pyf, dLa_v);
            if (BATCH) {
                if (recs) {
                    const int slot = slots[range.x + e];
                    if (slot >= 0 && (long long)slot < B.cap) {   // (a slot outside the frame's records is skipped, never written)
                        float *r = recs + (size_t)slot * (size_t)B.rec_stride;
#pragma unroll
                        for (int i = REC_UX; i < REC_O; ++i) atomic_add_f32(r + i, t.a[i] * t.b[i]);
                        if (!B.detach_opacity) atomic_add_f32(r + REC_O, t.a[REC_O] * t.b[REC_O]);
                    }
                }
            } else {
                if (A.dL_duv) {
                    atomic_add_f32(A.dL_duv + 2 * (size_t)id, t.a[REC_UX] * t.b[REC_UX]);
                    atomic_add_f32(A.dL_duv + 2 * (size_t)id + 1, t.a[REC_UY] * t.b[REC_UY]);
                }
                if (A.dL_dconic) {
                    atomic_add_f32(A.dL_dconic + 3 * (size_t)id, t.a[REC_CA] * t.b[REC_CA]);
                    atomic_add_f32(A.dL_dconic + 3 * (size_t)id + 1, t.a[REC_CB] * t.b[REC_CB]);
                    atomic_add_f32(A.dL_dconic + 3 * (size_t)id + 2, t.a[REC_CC] * t.b[REC_CC]);
                }
                if (A.dL_dopacity) atomic_add_f32(A.dL_dopacity + id, t.a[REC_O] * t.b[REC_O]);
            }
        }
    }
}

PointsBwdArgs points_bwd_args(int P, int C, const float *uv, const float *conic, const float *opacity, const float *feature,
                              const int32_t *idx_sorted, const int32_t *tile_range, float bg, int W, int H, const float *points,
                              const float *corner_T, const int32_t *corner_ncontrib, const float *dL_dout) {
    PointsBwdArgs A = points_args<PointsBwdArgs>(P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, points);
    A.corner_T = corner_T; A.corner_n = corner_ncontrib; A.dL_dout = dL_dout;
    return A;
}

// the launches of a validated atomic backward.  Every chunk adds its share of the geometry gradients: dL_dalpha is linear in the
// channels.
int points_backward(const PointsBwdArgs &A0, int Q, hipStream_t s, const PointsBatch *batch = nullptr) {
    const PointsBatch B = batch ? *batch : points_batch(0, 0, 0, nullptr, 0, 0, 0, 0);
    return points_chunks(A0, [&](const PointsBwdArgs &A, auto na) {
        constexpr int NA = decltype(na)::value;
        if (batch) SPLAT_LAUNCH("blend_points_bwd", (points_bwd_kernel<NA, true>), dim3((unsigned)Q), dim3(256), 0, s, A, B);
        else SPLAT_LAUNCH("blend_points_bwd", (points_bwd_kernel<NA, false>), dim3((unsigned)Q), dim3(256), 0, s, A, B);
    });
}

int points_refuse_deterministic(const char *fn, const char *instead) {
    splat_set_error("%s: deterministic mode: the backward of the sparse compositing adds with float atomics (many queries hit "
                    "one Gaussian); %s", fn, instead);
    return SPLAT_E_ARG;
}

// ---- the ORDERED backward: the same gradient without a float atomic, every sum in a fixed order.
// The atomic kernel above is one workgroup per query; here the (frame, tile) owns the work.  Every corner of a tile replays the
// same list, and every (Gaussian, tile) pair of that list has exactly one slot (slot_sorted of the pair map): the wave that owns
// a tile is the only writer of its slots and adds with plain loads and stores.
//   1. points_ord_corners_kernel<.., false>: thread = query; its LIVE corners (in the image, bilinear weight != 0,
//      corner_ncontrib > 0: points_bwd_kernel's exits, through the same points_corner) are counted per (frame, tile) with an INTEGER atomic (a count does
//      not depend on the arrival order);
//   2. points_ord_scan_kernel: exclusive scan of the counts (one workgroup);
//   3. points_ord_corners_kernel<.., true>: the corners' keys 4 q + k go into their tile's segment through an integer cursor,
//      in arrival order -- and points_ord_rank_kernel REORDERS every segment: the keys of a segment are unique, the rank of a
//      key among them is its place (thread = corner, one pass over its segment);
//   4. points_bwd_ordered_kernel: wave = (frame, tile) with corners (the others exit at once); it walks its corners in ascending
//      (q, k) and replays each with the machinery of points_bwd_kernel (lane = entry for 64 alphas, the applied entries back to
//      front with lane = channel, lane = entry for the geometry terms).  Every atomic_add_f32 of that kernel is here a load, an
//      add and a store BY THE SAME LANE on the same address (lane = channel for a feature column, lane = list position mod 64
//      for an entry's geometry terms), so program order fixes the sum: corners ascending, within a corner the entries back to
//      front.  Channel chunks are launches on one stream: ascending.
//   5. points_ord_gauss_kernel: thread = (Gaussian, column); sums the Gaussian's slots in ascending slot order (frames
//      ascending where the frames share the destination) from 0 and ADDS the sum to the caller's buffer.
struct PointsOrd {
    int NT;                         // F * T (frame, tile) owners
    int *seg;                       // [NT + 1]: the corners of every tile, then their exclusive scan (seg[NT] = all live corners)
    int *cursor;                    // [NT]
    int *tmp_key, *tmp_tile;        // [4 Q]: the corners in arrival order
    int *sorted;                    // [4 Q]: every tile's keys 4 q + k ascending
    // where an applied entry with slot s of frame f adds: geometry at geo + f geo_fs + s geo_stride + REC_*, feature column c at
    // fsc + f fsc_fs + s fsc_stride + c (fsc already points at the first feature column); either may be NULL
    float *geo, *fsc;
    long long geo_stride, geo_fs, fsc_stride, fsc_fs;
};

// corner k of a query at pt: the tile of a live corner, else -1
__device__ __forceinline__ int points_live_corner_tile(const PointsBwdArgs &A, size_t q, float2 pt, int k) {
    const PointsCorner K = points_corner(pt, k, A.W, A.H);
    if (!K.in || K.cw == 0.f) return -1;
    if (A.corner_n[q * 4 + k] <= 0) return -1;
    return K.ty * A.gx + K.tx;
}

template <bool BATCH, bool FILL>
__global__ void __launch_bounds__(256) points_ord_corners_kernel(const PointsBwdArgs A, const PointsBatch B, const PointsOrd O) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= B.Q) return;
    int f = 0;
    if (BATCH) {
        f = points_frame_of(B, q);
        if (f < 0) return;   // a query no frame owns
    }
    const float2 pt = A.points[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tile = points_live_corner_tile(A, (size_t)q, pt, k);
        if (tile < 0) continue;
        const int t = f * B.T + tile;
        if (!FILL) {
            atomicAdd(O.seg + t, 1);
        } else {   // (arrival order: points_ord_rank_kernel reorders the segment)
            const int pos = O.seg[t] + atomicAdd(O.cursor + t, 1);
            O.tmp_key[pos] = (int)(4 * q + k);
            O.tmp_tile[pos] = t;
        }
    }
}

// seg[0 .. n) -> its exclusive scan in place, seg[n] = the total.  One workgroup: n = F T is some ten thousand.
__global__ void __launch_bounds__(1024) points_ord_scan_kernel(int *seg, int n) {
    __shared__ int s[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const long long b = (long long)tid * per;
    const long long e = b + per < n ? b + per : n;
    int sum = 0;
    for (long long i = b; i < e; ++i) sum += seg[i];
    s[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    int run = s[tid] - sum;
    for (long long i = b; i < e; ++i) {
        const int c = seg[i];
        seg[i] = run;
        run += c;
    }
    if (tid == 1023) seg[n] = s[1023];
}

// thread = corner in arrival order: its rank among the (unique) keys of its tile's segment is its place
__global__ void __launch_bounds__(256) points_ord_rank_kernel(const PointsOrd O) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= O.seg[O.NT]) return;
    const int t = O.tmp_tile[i], key = O.tmp_key[i];
    const int s0 = O.seg[t], s1 = O.seg[t + 1];
    int r = 0;
    for (int j = s0; j < s1; ++j) r += O.tmp_key[j] < key ? 1 : 0;
    O.sorted[s0 + r] = key;
}

template <int NA>
__global__ void __launch_bounds__(256) points_bwd_ordered_kernel(const PointsBwdArgs A0, const PointsBatch B, const PointsOrd O) {
    const int tid = threadIdx.x, lane = tid & 63;
    const long long gw = (long long)blockIdx.x * 4 + (tid >> 6);
    if (gw >= O.NT) return;
    const int t = __builtin_amdgcn_readfirstlane((int)gw);   // wave = (frame, tile): everything below branches on scalars
    const int s0 = __builtin_amdgcn_readfirstlane(O.seg[t]), s1 = __builtin_amdgcn_readfirstlane(O.seg[t + 1]);
    if (s0 >= s1) return;   // a tile without live corners
    const int f = t / B.T, tile = t - f * B.T;
    PointsBwdArgs A = A0;
    points_frame_view(A, B, f);
    const int *slots = B.slot_sorted + (size_t)f * (size_t)B.cap;
    float *geo = O.geo ? O.geo + (size_t)f * (size_t)O.geo_fs : nullptr;
    float *dfbase = O.fsc ? O.fsc + (size_t)f * (size_t)O.fsc_fs + A.c0 + lane : nullptr;
    const int2 range = A.tile_range[tile];
    // (a list that leaves the frame's segment is cut short, never read)
    long long nn = (long long)range.y - (long long)range.x;
    nn = nn > B.cap - (long long)range.x ? B.cap - (long long)range.x : nn;
    const int n = range.x < 0 || nn < 0 ? 0 : (int)nn;
    const float *fbase = A.feature + A.c0 + lane;

    for (int ci = s0; ci < s1; ++ci) {   // the tile's live corners in ascending (q, k)
        const int key = __builtin_amdgcn_readfirstlane(O.sorted[ci]);
        const size_t q = (size_t)(key >> 2);
        const int w = key & 3;
        const float2 ptv = A.points[q];
        // (the corner is live: inside the image, cw != 0, and its pixel lies in this tile)
        const PointsCorner K = points_corner(make_float2(lane_f(ptv.x, 0), lane_f(ptv.y, 0)), w, A.W, A.H);
        const float cw = K.cw;
        const int last = imin_(__builtin_amdgcn_readfirstlane(A.corner_n[q * 4 + w]), n);   // (never past the list)
        if (last <= 0) continue;
        const float Tf = lane_f(A.corner_T[q * 4 + w], 0);
        const float pxf = (float)K.px, pyf = (float)K.py;

        float g[NA], acc[NA];
        float gsum = 0.f;
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            g[k] = (lane + 64 * k < A.cn) ? cw * A.dL_dout[q * (size_t)A.C + A.c0 + lane + 64 * k] : 0.f;
            acc[k] = 0.f;
            gsum += g[k];
        }
        const float bgdot = A.bg * wave_sum_bcast(gsum);
        float T = Tf;

        for (int base = ((last - 1) / WAVE) * WAVE; base >= 0; base -= WAVE) {
            // ---- lane = entry: its alpha on this pixel (the forward's bits) and its slot
            const int e = base + lane;
            PointsEntry E;
            const bool aok = points_entry(A, K, range.x, e, last, E, slots);
            const int id = E.id;
            const float alpha = E.alpha;
            const int slot = (long long)E.slot < B.cap ? E.slot : -1;   // (a slot outside the frame's records is skipped, never written)
            // ---- lane = channel: the applied entries back to front, four rows in flight
            unsigned long long ap = __ballot(aok);
            float dLa_v = 0.f;   // lane j: dL_dalpha of entry base + j, if it applied
            while (ap) {
                int jj[4];
                float fr[4][NA], dr[4][NA];   // feature rows and the slots' running feature sums (distinct entries of a list have
                float *drow[4];               //   distinct slots: the four rows do not alias)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    jj[u] = ap ? 63 - (int)__builtin_clzll(ap) : -1;
                    drow[u] = nullptr;
#pragma unroll
                    for (int k = 0; k < NA; ++k) fr[u][k] = dr[u][k] = 0.f;
                    if (jj[u] >= 0) {
                        ap &= ~(1ull << jj[u]);
                        const float *row = fbase + (size_t)__builtin_amdgcn_readlane(id, jj[u]) * (size_t)A.C;
#pragma unroll
                        for (int k = 0; k < NA; ++k) fr[u][k] = (lane + 64 * k < A.cn) ? row[64 * k] : 0.f;
                        const int sj = __builtin_amdgcn_readlane(slot, jj[u]);
                        if (dfbase && sj >= 0) {
                            drow[u] = dfbase + (size_t)sj * (size_t)O.fsc_stride;
#pragma unroll
                            for (int k = 0; k < NA; ++k) dr[u][k] = (lane + 64 * k < A.cn) ? drow[u][64 * k] : 0.f;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (jj[u] < 0) break;
                    const int j = jj[u];
                    const float a = lane_f(alpha, j);
                    const float r1a = __builtin_amdgcn_rcpf(1.f - a);
                    T = T * r1a;   // the transmittance in front of the entry
                    const float wgt = a * T;
                    float part = 0.f;
#pragma unroll
                    for (int k = 0; k < NA; ++k) part += (fr[u][k] - acc[k]) * g[k];
                    float dLa = wave_sum_bcast(part) * T;
                    dLa += (-Tf * r1a) * bgdot;
                    dLa_v = lane == j ? dLa : dLa_v;
                    if (drow[u]) {   // this lane is the only writer of its column of the slot: loaded above, add, store
#pragma unroll
                        for (int k = 0; k < NA; ++k)
                            if (lane + 64 * k < A.cn) drow[u][64 * k] = dr[u][k] + wgt * g[k];
                    }
#pragma unroll
                    for (int k = 0; k < NA; ++k) acc[k] = a * fr[u][k] + (1.f - a) * acc[k];
                }
            }
            // ---- lane = entry: the geometry terms of the block's applied entries (replay_one's expressions); list position e is
            //      this lane's in every corner of the tile, and its slot is nobody else's
            if (aok && geo && slot >= 0) {
                const PointsGeoTerms t = points_geo_terms(E, pxf, pyf, dLa_v);
                float *r = geo + (size_t)slot * (size_t)O.geo_stride;
#pragma unroll
                for (int i = REC_UX; i < REC_O; ++i) r[i] = r[i] + t.a[i] * t.b[i];
                if (!B.detach_opacity) r[REC_O] = r[REC_O] + t.a[REC_O] * t.b[REC_O];
            }
        }
    }
}

// thread = (Gaussian i, column j of the slot records at `sc`, `stride` floats apart, `fs` floats per frame): the sum of the
// Gaussian's slots [goff_incl[f, i - 1], goff_incl[f, i]) in ascending order from 0, frames ascending, ADDED to its destination.
// geom: columns 0 .. 5 are ux uy ca cb cc o (-> dL_duv, dL_dconic, dL_dopacity), the feature columns follow; else all columns
// are feature columns.  dfeat_fs != 0: every frame's feature sum goes to its own block.
__global__ void __launch_bounds__(256) points_ord_gauss_kernel(int F, int P, int ncol, const float *sc, long long stride, long long fs,
                                                               long long cap, const int *goff, int geom, float *duv, float *dconic,
                                                               float *dopac, float *dfeat, int C, long long dfeat_fs) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)P * (size_t)ncol) return;
    const size_t i = idx / (size_t)ncol;
    const int j = (int)(idx - i * (size_t)ncol);
    const bool isgeo = geom && j < REC_GEOM;
    float *dst = nullptr;
    if (isgeo) {
        if (j < 2) dst = duv ? duv + 2 * i + j : nullptr;
        else if (j < 5) dst = dconic ? dconic + 3 * i + (j - 2) : nullptr;
        else dst = dopac ? dopac + i : nullptr;
    } else {
        dst = dfeat ? dfeat + i * (size_t)C + (j - (geom ? REC_GEOM : 0)) : nullptr;
    }
    if (!dst) return;
    const bool per_frame = !isgeo && dfeat_fs != 0;
    float sum = 0.f;
    for (int f = 0; f < F; ++f) {
        const int *g = goff + (size_t)f * (size_t)P;
        long long a = i ? g[i - 1] : 0, b = g[i];
        a = a < 0 ? 0 : a;
        b = b > cap ? cap : b;   // (slots past the capacity do not exist)
        const float *col = sc + (size_t)f * (size_t)fs + j;
        for (long long s = a; s < b; ++s) sum += col[(size_t)s * (size_t)stride];
        if (per_frame) {
            dst[(size_t)f * (size_t)dfeat_fs] += sum;
            sum = 0.f;
        }
    }
    if (!per_frame) *dst += sum;
}

struct OrdLayout {
    size_t seg, cursor, tmp_key, tmp_tile, sorted, rec, total;   // byte offsets into the scratch
};

// [seg NT + 1 | cursor NT | three int arrays of 4 Q] rounded up to 16 bytes, then `rec_floats` floats of slot records
bool points_ord_layout(long long NT, long long Q, double rec_floats, OrdLayout &L) {
    if (NT < 1 || Q < 0 || !(rec_floats >= 0.0 && rec_floats < 4.0e18 / 4.0)) return false;
    const size_t nt = (size_t)NT, q4 = 4 * (size_t)Q;
    L.seg = 0;
    L.cursor = 4 * (nt + 1);
    L.tmp_key = L.cursor + 4 * nt;
    L.tmp_tile = L.tmp_key + 4 * q4;
    L.sorted = L.tmp_tile + 4 * q4;
    L.rec = (L.sorted + 4 * q4 + 15) & ~(size_t)15;
    L.total = L.rec + 4 * (size_t)rec_floats;
    return true;
}

// the launches of a validated ordered backward.  A / B as the atomic entries fill them (single frame: F = 1, no offsets).
int points_ordered_run(const PointsBwdArgs &A, const PointsBatch &B, PointsOrd O, bool batch, const OrdLayout &L, char *scratch,
                       size_t rec_bytes_to_zero, hipStream_t s) {
    const int Q = (int)B.Q;
    O.seg = (int *)(scratch + L.seg); O.cursor = (int *)(scratch + L.cursor);
    O.tmp_key = (int *)(scratch + L.tmp_key); O.tmp_tile = (int *)(scratch + L.tmp_tile); O.sorted = (int *)(scratch + L.sorted);
    {
        ProfiledLaunch pl_("blend_points_ord_zero", s);
        SPLAT_CHECK_HIP(hipMemsetAsync(scratch, 0, L.tmp_key, s));   // counts and cursors
        if (rec_bytes_to_zero) SPLAT_CHECK_HIP(hipMemsetAsync(scratch + L.rec, 0, rec_bytes_to_zero, s));   // the slot records
    }
    const dim3 qgrid((unsigned)(((size_t)Q + 255) / 256)), cgrid((unsigned)((4 * (size_t)Q + 255) / 256));
    if (batch) SPLAT_LAUNCH("blend_points_ord_lists", (points_ord_corners_kernel<true, false>), qgrid, dim3(256), 0, s, A, B, O);
    else SPLAT_LAUNCH("blend_points_ord_lists", (points_ord_corners_kernel<false, false>), qgrid, dim3(256), 0, s, A, B, O);
    SPLAT_POST_LAUNCH();
    SPLAT_LAUNCH("blend_points_ord_lists", points_ord_scan_kernel, dim3(1), dim3(1024), 0, s, O.seg, O.NT);
    SPLAT_POST_LAUNCH();
    if (batch) SPLAT_LAUNCH("blend_points_ord_lists", (points_ord_corners_kernel<true, true>), qgrid, dim3(256), 0, s, A, B, O);
    else SPLAT_LAUNCH("blend_points_ord_lists", (points_ord_corners_kernel<false, true>), qgrid, dim3(256), 0, s, A, B, O);
    SPLAT_POST_LAUNCH();
    SPLAT_LAUNCH("blend_points_ord_lists", points_ord_rank_kernel, cgrid, dim3(256), 0, s, O);
    SPLAT_POST_LAUNCH();
    const dim3 tgrid((unsigned)(((size_t)O.NT + 3) / 4));
    // every chunk adds its share of the geometry terms: dL_dalpha is linear in the channels
    return points_chunks(A, [&](const PointsBwdArgs &a, auto na) {
        SPLAT_LAUNCH("blend_points_bwd_ord", points_bwd_ordered_kernel<decltype(na)::value>, tgrid, dim3(256), 0, s, a, B, O);
    });
}

// rows[n, t] = (u_t - u_ref, v_t - v_ref, depth_t) of Gaussian n at the t-th time of the table: get_position(t) (the segment
// polynomial of dynamic_eval_fwd_kernel) through the orthographic project_point.  One thread per (n, t): consecutive threads
// write consecutive 12-byte entries of a Gaussian's row.
__global__ void __launch_bounds__(DYN_BLOCK) track_flow_rows_kernel(int T, int P, int I, int layout, const DynTab *__restrict__ tab,
                                                                    const float *__restrict__ position, const float *__restrict__ cubic,
                                                                    const float *__restrict__ extr, int W, int H, float nearest,
                                                                    float extent, int no_cull, const float2 *__restrict__ uv_ref,
                                                                    float *__restrict__ rows) {
    const size_t i = (size_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
    if (i >= (size_t)P * (size_t)T) return;
    const size_t n = i / (size_t)T;
    const int t = (int)(i - n * (size_t)T);
    const int seg = imin_(imax_(tab[t].seg, 0), I - 1);   // (a segment outside the table is clamped, never dereferenced)
    const CubicAddr ca = cubic_addr(layout, P, I, seg);
    const float d = tab[t].d;
    float p3[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float *c = cubic + ca.seg_off + n * ca.stride_n + j;
        const size_t row = ca.stride_k;
        const float c0 = c[0], c1 = c[row], c2 = c[2 * row], c3 = c[3 * row];
        float p = c3 + c2 * d;
        p = p + c1 * (d * d);
        p = p + c0 * (d * d * d);
        p3[j] = p + position[n * 3 + j];
    }
    Cam cam;
    load_cam(nullptr, extr, cam);
    float u, v, dep;
    const bool cull = project_ortho_pt(cam, p3[0], p3[1], p3[2], W, H, nearest, extent, u, v, dep) && !no_cull;
    u = cull ? 0.f : u; v = cull ? 0.f : v; dep = cull ? 0.f : dep;
    const float2 r = uv_ref[n];
    float *o = rows + i * 3;
    o[0] = u - r.x;
    o[1] = v - r.y;
    o[2] = dep;
}

}  // namespace

extern "C" int splat_alpha_blending_points_forward(int P, int C, const float *uv, const float *conic, const float *opacity,
                                                   const float *feature, const int32_t *idx_sorted, const int32_t *tile_range,
                                                   float bg, int W, int H, int Q, const float *points, float *out,
                                                   float *corner_T, int32_t *corner_ncontrib, splat_stream_t stream) {
    return points_forward_entry(__func__, false, P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, Q, points, out,
                                corner_T, corner_ncontrib, stream);
}

extern "C" int splat_alpha_blending_points_forward_live(int P, int C, const float *uv, const float *conic, const float *opacity,
                                                        const float *feature, const int32_t *idx_sorted, const int32_t *tile_range,
                                                        float bg, int W, int H, int Q, const float *points, float *out,
                                                        float *corner_T, int32_t *corner_ncontrib, splat_stream_t stream) {
    return points_forward_entry(__func__, true, P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, Q, points, out,
                                corner_T, corner_ncontrib, stream);
}

extern "C" int splat_alpha_blending_points_backward(int P, int C, const float *uv, const float *conic, const float *opacity,
                                                    const float *feature, const int32_t *idx_sorted, const int32_t *tile_range,
                                                    float bg, int W, int H, int Q, const float *points, const float *corner_T,
                                                    const int32_t *corner_ncontrib, const float *dL_dout, float *dL_duv,
                                                    float *dL_dconic, float *dL_dopacity, float *dL_dfeature, splat_stream_t stream) {
    SPLAT_CHECK_ARG(P >= 0 && C >= 1 && W > 0 && H > 0 && Q >= 0, "bad sizes (P, Q >= 0, C, W, H >= 1)");
    SPLAT_CHECK_ARG(W <= (1 << 24) && H <= (1 << 24), "sizes too large (W, H <= 2^24: pixel indices are compared in float32)");
    if (Q == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(points && corner_T && corner_ncontrib && dL_dout, "null pointer (points / corner_T / corner_ncontrib / dL_dout)");
    SPLAT_CHECK_ARG(P == 0 || (uv && conic && opacity && feature && tile_range), "null pointer");
    if (P == 0 || !(dL_duv || dL_dconic || dL_dopacity || dL_dfeature)) return SPLAT_OK;   // nothing to add to
    if (splat_deterministic()) return points_refuse_deterministic(__func__, "use the dense alpha_blending route");   // before any launch
    PointsBwdArgs A = points_bwd_args(P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, points, corner_T,
                                      corner_ncontrib, dL_dout);
    A.dL_duv = dL_duv; A.dL_dconic = dL_dconic; A.dL_dopacity = dL_dopacity; A.dL_dfeature = dL_dfeature;
    return points_backward(A, Q, (hipStream_t)stream);
}

// ---- the frame-batched entries: the queries of F frames of a FrameBatch in one launch per 256-channel chunk
namespace {
int points_batch_check(const char *fn, int F, int P, int C, int W, int H, int64_t Q, int64_t capacity, int64_t opacity_fs,
                       int64_t feature_fs) {
    PT_CHECK(fn, F >= 1 && P >= 0 && C >= 1 && W > 0 && H > 0 && Q >= 0 && capacity >= 0 && opacity_fs >= 0 && feature_fs >= 0,
             "bad sizes (F, C, W, H >= 1; P, Q, capacity, frame strides >= 0)");
    PT_CHECK(fn, W <= (1 << 24) && H <= (1 << 24) && Q <= 0x7fffffffLL && F <= (1 << 16),
             "sizes too large (W, H <= 2^24: pixel indices are compared in float32; Q < 2^31, F <= 2^16)");
    return SPLAT_OK;
}

// the size checks that the two batch backward entries add
int points_batch_bwd_check(const char *fn, int64_t dfeature_fs, const float *pair_records, int record_stride, int64_t capacity) {
    PT_CHECK(fn, dfeature_fs >= 0, "bad sizes (dL_dfeature frame stride >= 0)");
    PT_CHECK(fn, !pair_records || (record_stride >= REC_GEOM && record_stride % 4 == 0 && capacity >= 1),
             "bad sizes (pair records: a stride of whole 16-byte chunks >= 8 floats, capacity >= 1)");
    return SPLAT_OK;
}

PointsBatch points_batch_bwd(int F, int W, int H, const int64_t *offsets, int64_t Q, int64_t capacity, int64_t opacity_fs,
                             int64_t feature_fs, int64_t dfeature_fs, const int32_t *slot_sorted, float *pair_records,
                             int record_stride, int detach_opacity) {
    PointsBatch B = points_batch(F, W, H, offsets, Q, capacity, opacity_fs, feature_fs);
    B.dfeature_fs = dfeature_fs;
    B.slot_sorted = slot_sorted; B.rec = pair_records; B.rec_stride = record_stride; B.detach_opacity = detach_opacity ? 1 : 0;
    return B;
}
}  // namespace

extern "C" int splat_alpha_blending_points_forward_batch(int F, int P, int C, const float *uv, const float *conic,
                                                         const float *opacity, int64_t opacity_frame_stride, const float *feature,
                                                         int64_t feature_frame_stride, const int32_t *idx_sorted,
                                                         const int32_t *tile_range, int64_t capacity, float bg, int W, int H,
                                                         int64_t Q, const int64_t *offsets, const float *points, float *out,
                                                         float *corner_T, int32_t *corner_ncontrib, splat_stream_t stream) {
    const int rc = points_batch_check(__func__, F, P, C, W, H, Q, capacity, opacity_frame_stride, feature_frame_stride);
    if (rc != SPLAT_OK) return rc;
    if (Q == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(points && out && offsets, "null pointer (points / out / offsets)");
    SPLAT_CHECK_ARG(P == 0 || (uv && conic && opacity && feature && tile_range), "null pointer");
    const PointsBatch B = points_batch(F, W, H, offsets, Q, capacity, opacity_frame_stride, feature_frame_stride);
    PointsArgs A = points_args<PointsArgs>(P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, points);
    A.out = out; A.corner_T = corner_T; A.corner_n = corner_ncontrib;
    return points_forward(A, (int)Q, true, (hipStream_t)stream, &B);
}

// RELIES ON: (1) corner_T / corner_ncontrib of splat_alpha_blending_points_forward_batch on the same buffers; (2) the tile
// backward of the SAME forward (splat_alpha_blending_backward_batch_sets* / _batch) has run on this stream and has WRITTEN every
// record of every frame's used slots -- each variant stores the combined record of the entries it replays and a zero record for
// the entries nobody replays, so this entry only ever adds to initialised floats; (3) the Gaussian-side backward
// (splat_frames_gauss_backward_*), which sums a Gaussian's records, runs after it.
extern "C" int splat_alpha_blending_points_backward_batch(int F, int P, int C, const float *uv, const float *conic,
                                                          const float *opacity, int64_t opacity_frame_stride, const float *feature,
                                                          int64_t feature_frame_stride, const int32_t *idx_sorted,
                                                          const int32_t *tile_range, int64_t capacity, float bg, int W, int H,
                                                          int64_t Q, const int64_t *offsets, const float *points,
                                                          const float *corner_T, const int32_t *corner_ncontrib,
                                                          const float *dL_dout, const int32_t *slot_sorted, float *pair_records,
                                                          int record_stride, int detach_opacity, float *dL_dfeature,
                                                          int64_t dfeature_frame_stride, splat_stream_t stream) {
    int rc = points_batch_check(__func__, F, P, C, W, H, Q, capacity, opacity_frame_stride, feature_frame_stride);
    if (rc != SPLAT_OK) return rc;
    rc = points_batch_bwd_check(__func__, dfeature_frame_stride, pair_records, record_stride, capacity);
    if (rc != SPLAT_OK) return rc;
    if (Q == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(points && offsets && corner_T && corner_ncontrib && dL_dout,
                    "null pointer (points / offsets / corner_T / corner_ncontrib / dL_dout)");
    SPLAT_CHECK_ARG(P == 0 || (uv && conic && opacity && feature && tile_range), "null pointer");
    SPLAT_CHECK_ARG(!pair_records || slot_sorted, "null pointer (slot_sorted goes with pair_records)");
    if (P == 0 || !(pair_records || dL_dfeature)) return SPLAT_OK;   // nothing to add to
    SPLAT_CHECK_ARG(idx_sorted, "null pointer (idx_sorted)");
    if (splat_deterministic()) return points_refuse_deterministic(__func__, "render the set densely instead");   // before any launch
    const PointsBatch B = points_batch_bwd(F, W, H, offsets, Q, capacity, opacity_frame_stride, feature_frame_stride,
                                           dfeature_frame_stride, slot_sorted, pair_records, record_stride, detach_opacity);
    PointsBwdArgs A = points_bwd_args(P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, points, corner_T,
                                      corner_ncontrib, dL_dout);
    A.dL_dfeature = dL_dfeature;
    return points_backward(A, (int)Q, (hipStream_t)stream, &B);
}

// ---- the ordered entries: no float atomic, run with the deterministic flag on or off
namespace {
constexpr long long ORD_MAX_Q = 1ll << 29;    // a corner's key 4 q + k is an int32
constexpr long long ORD_MAX_NT = 1ll << 30;   // (frame, tile) owners

int points_ord_gauss(int F, int P, int ncol, const float *sc, long long stride, long long fs, long long cap, const int32_t *goff,
                     int geom, float *duv, float *dconic, float *dopac, float *dfeat, int C, long long dfeat_fs, hipStream_t s) {
    const size_t total = (size_t)P * (size_t)ncol;
    SPLAT_LAUNCH("blend_points_ord_gauss", points_ord_gauss_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, F, P, ncol,
                 sc, stride, fs, cap, goff, geom, duv, dconic, dopac, dfeat, C, dfeat_fs);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}
}  // namespace

extern "C" size_t splat_alpha_blending_points_backward_ordered_scratch_bytes(int C, int W, int H, int Q, int64_t capacity) {
    if (!(C >= 1 && W > 0 && H > 0 && Q >= 0 && capacity >= 0)) return 0;
    if (!(W <= (1 << 24) && H <= (1 << 24) && Q <= ORD_MAX_Q && points_num_tiles(W, H) <= ORD_MAX_NT)) return 0;
    OrdLayout L;
    if (!points_ord_layout(points_num_tiles(W, H), Q, (double)capacity * (double)PAIR_STRIDE(REC_GEOM + (long long)C), L)) return 0;
    return L.total;
}

extern "C" size_t splat_alpha_blending_points_backward_batch_ordered_scratch_bytes(int F, int C, int W, int H, int64_t Q,
                                                                                   int64_t capacity) {
    if (!(F >= 1 && C >= 1 && W > 0 && H > 0 && Q >= 0 && capacity >= 0)) return 0;
    if (!(W <= (1 << 24) && H <= (1 << 24) && Q <= ORD_MAX_Q && F <= (1 << 16) && (long long)F * points_num_tiles(W, H) <= ORD_MAX_NT))
        return 0;
    OrdLayout L;
    if (!points_ord_layout((long long)F * points_num_tiles(W, H), Q, (double)F * (double)capacity * (double)PAIR_STRIDE((long long)C), L))
        return 0;
    return L.total;
}

extern "C" int splat_alpha_blending_points_backward_ordered(int P, int C, const float *uv, const float *conic, const float *opacity,
                                                            const float *feature, const int32_t *idx_sorted,
                                                            const int32_t *tile_range, int64_t capacity, float bg, int W, int H, int Q,
                                                            const float *points, const float *corner_T,
                                                            const int32_t *corner_ncontrib, const float *dL_dout, float *dL_duv,
                                                            float *dL_dconic, float *dL_dopacity, float *dL_dfeature,
                                                            const int32_t *goff_incl, const int32_t *slot_sorted, void *scratch,
                                                            size_t scratch_bytes, splat_stream_t stream) {
    SPLAT_CHECK_ARG(P >= 0 && C >= 1 && W > 0 && H > 0 && Q >= 0 && capacity >= 0, "bad sizes (P, Q, capacity >= 0, C, W, H >= 1)");
    SPLAT_CHECK_ARG(W <= (1 << 24) && H <= (1 << 24) && Q <= ORD_MAX_Q && points_num_tiles(W, H) <= ORD_MAX_NT,
                    "sizes too large (W, H <= 2^24: pixel indices are compared in float32; Q <= 2^29, tiles <= 2^30)");
    if (Q == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(points && corner_T && corner_ncontrib && dL_dout, "null pointer (points / corner_T / corner_ncontrib / dL_dout)");
    SPLAT_CHECK_ARG(P == 0 || (uv && conic && opacity && feature && tile_range), "null pointer");
    if (P == 0 || !(dL_duv || dL_dconic || dL_dopacity || dL_dfeature)) return SPLAT_OK;   // nothing to add to
    SPLAT_CHECK_ARG(goff_incl && slot_sorted, "the ordered backward needs this library's pair map (goff_incl, slot_sorted of "
                                              "splat_bin_sort for THIS idx_sorted); a foreign idx_sorted has none");
    SPLAT_CHECK_ARG(idx_sorted, "null pointer (idx_sorted)");
    const size_t need = splat_alpha_blending_points_backward_ordered_scratch_bytes(C, W, H, Q, capacity);
    SPLAT_CHECK_ARG(need != 0, "sizes too large (scratch)");
    SPLAT_CHECK_ARG(scratch && scratch_bytes >= need,
                    "scratch missing or too small (splat_alpha_blending_points_backward_ordered_scratch_bytes)");
    if (capacity == 0) return SPLAT_OK;   // no pair, no slot: every list is empty
    const int T = (int)points_num_tiles(W, H);
    const int S = PAIR_STRIDE(REC_GEOM + C);
    OrdLayout L;
    points_ord_layout(T, Q, (double)capacity * (double)S, L);
    PointsBatch B = points_batch(1, W, H, nullptr, Q, capacity, 0, 0);
    B.slot_sorted = slot_sorted;
    const PointsBwdArgs A = points_bwd_args(P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, points, corner_T,
                                            corner_ncontrib, dL_dout);
    float *rec = (float *)((char *)scratch + L.rec);
    PointsOrd O;
    memset(&O, 0, sizeof(O));
    O.NT = T;
    if (dL_duv || dL_dconic || dL_dopacity) { O.geo = rec; O.geo_stride = S; }
    if (dL_dfeature) { O.fsc = rec + REC_GEOM; O.fsc_stride = S; }
    const int rc = points_ordered_run(A, B, O, false, L, (char *)scratch, (size_t)capacity * (size_t)S * 4, (hipStream_t)stream);
    if (rc != SPLAT_OK) return rc;
    return points_ord_gauss(1, P, REC_GEOM + C, rec, S, 0, capacity, goff_incl, 1, dL_duv, dL_dconic, dL_dopacity, dL_dfeature, C, 0,
                            (hipStream_t)stream);
}

// RELIES ON what splat_alpha_blending_points_backward_batch relies on (corner maps of the batch forward, the tile backward of the
// same forward before it, the Gaussian-side backward after it).
extern "C" int splat_alpha_blending_points_backward_batch_ordered(
    int F, int P, int C, const float *uv, const float *conic, const float *opacity, int64_t opacity_frame_stride, const float *feature,
    int64_t feature_frame_stride, const int32_t *idx_sorted, const int32_t *tile_range, int64_t capacity, float bg, int W, int H,
    int64_t Q, const int64_t *offsets, const float *points, const float *corner_T, const int32_t *corner_ncontrib,
    const float *dL_dout, const int32_t *slot_sorted, float *pair_records, int record_stride, int detach_opacity, float *dL_dfeature,
    int64_t dfeature_frame_stride, const int32_t *goff_incl, void *scratch, size_t scratch_bytes, splat_stream_t stream) {
    int rc = points_batch_check(__func__, F, P, C, W, H, Q, capacity, opacity_frame_stride, feature_frame_stride);
    if (rc != SPLAT_OK) return rc;
    SPLAT_CHECK_ARG(Q <= ORD_MAX_Q && (long long)F * points_num_tiles(W, H) <= ORD_MAX_NT,
                    "sizes too large (Q <= 2^29, F * tiles <= 2^30)");
    rc = points_batch_bwd_check(__func__, dfeature_frame_stride, pair_records, record_stride, capacity);
    if (rc != SPLAT_OK) return rc;
    if (Q == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(points && offsets && corner_T && corner_ncontrib && dL_dout,
                    "null pointer (points / offsets / corner_T / corner_ncontrib / dL_dout)");
    SPLAT_CHECK_ARG(P == 0 || (uv && conic && opacity && feature && tile_range), "null pointer");
    if (P == 0 || !(pair_records || dL_dfeature)) return SPLAT_OK;   // nothing to add to
    SPLAT_CHECK_ARG(goff_incl && slot_sorted, "the ordered backward needs the frame batch's pair map (goff_incl [F, P], slot_sorted "
                                              "[F, capacity] of splat_bin_sort_batch for THIS idx_sorted)");
    SPLAT_CHECK_ARG(idx_sorted, "null pointer (idx_sorted)");
    const size_t need = splat_alpha_blending_points_backward_batch_ordered_scratch_bytes(F, C, W, H, Q, capacity);
    SPLAT_CHECK_ARG(need != 0, "sizes too large (scratch)");
    SPLAT_CHECK_ARG(scratch && scratch_bytes >= need,
                    "scratch missing or too small (splat_alpha_blending_points_backward_batch_ordered_scratch_bytes)");
    if (capacity == 0) return SPLAT_OK;   // no pair, no slot: every list is empty
    const int T = (int)points_num_tiles(W, H);
    const int S = PAIR_STRIDE(C);
    OrdLayout L;
    points_ord_layout((long long)F * T, Q, (double)F * (double)capacity * (double)S, L);
    const PointsBatch B = points_batch_bwd(F, W, H, offsets, Q, capacity, opacity_frame_stride, feature_frame_stride,
                                           dfeature_frame_stride, slot_sorted, pair_records, record_stride, detach_opacity);
    const PointsBwdArgs A = points_bwd_args(P, C, uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, points, corner_T,
                                            corner_ncontrib, dL_dout);
    float *rec = (float *)((char *)scratch + L.rec);
    PointsOrd O;
    memset(&O, 0, sizeof(O));
    O.NT = F * T;
    if (pair_records) { O.geo = pair_records; O.geo_stride = record_stride; O.geo_fs = (long long)capacity * record_stride; }
    if (dL_dfeature) { O.fsc = rec; O.fsc_stride = S; O.fsc_fs = (long long)capacity * S; }
    const size_t zero = dL_dfeature ? (size_t)F * (size_t)capacity * (size_t)S * 4 : 0;
    rc = points_ordered_run(A, B, O, true, L, (char *)scratch, zero, (hipStream_t)stream);
    if (rc != SPLAT_OK) return rc;
    if (!dL_dfeature) return SPLAT_OK;
    return points_ord_gauss(F, P, C, rec, S, (long long)capacity * S, capacity, goff_incl, 0, nullptr, nullptr, nullptr, dL_dfeature, C,
                            dfeature_frame_stride, (hipStream_t)stream);
}

extern "C" int splat_track_flow_rows(int T, int P, int I, const void *tab, const float *position, const float *cubic,
                                     int cubic_layout, const float *extr, int W, int H, float nearest, float extent,
                                     const float *uv_ref, float *rows, splat_stream_t stream) {
    SPLAT_CHECK_ARG(T >= 0 && P >= 0 && I >= 1 && W > 0 && H > 0, "bad sizes (T, P >= 0, I, W, H >= 1)");
    SPLAT_CHECK_ARG(cubic_layout == SPLAT_CUBIC_GAUSSIAN_MAJOR || cubic_layout == SPLAT_CUBIC_SEGMENT_MAJOR, "unknown cubic_layout");
    SPLAT_CHECK_ARG(nearest == nearest && extent == extent, "nearest / extent must not be NaN");
    if (T == 0 || P == 0) return SPLAT_OK;
    SPLAT_CHECK_ARG(tab && position && cubic && extr && uv_ref && rows, "null pointer");
    const size_t total = (size_t)P * (size_t)T;
    SPLAT_CHECK_ARG((total + DYN_BLOCK - 1) / DYN_BLOCK <= 0x7fffffffull, "sizes too large");
    const int no_cull = (nearest == 0.f && extent == 0.f) ? 1 : 0;   // nearest = extent = 0: culling switched off
    SPLAT_LAUNCH("track_flow_rows", track_flow_rows_kernel, dim3((unsigned)((total + DYN_BLOCK - 1) / DYN_BLOCK)), dim3(DYN_BLOCK), 0,
                 (hipStream_t)stream, T, P, I, cubic_layout, (const DynTab *)tab, position, cubic, extr, W, H, nearest, extent, no_cull,
                 (const float2 *)uv_ref, rows);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}
