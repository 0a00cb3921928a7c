// Camera gradients of a frame batch of dynamic Gaussians (include/splat_hip_camera_grad.h): dL/dextr per frame and, under the
// pinhole camera, dL/dintr, from the pair records the Gaussian-side walk (gauss_dyn_bwd.h) reads.  A kernel of its own beside
// the walk: there every lane keeps another frame, so a per-frame sum over the Gaussians would cost a workgroup reduction on
// every four-frame trip and sixteen more accumulators per lane.  No float atomics: two launches (three for a shared camera),
// a fixed order of every sum.
#include "gauss_dyn_bwd.h"
#include "../../include/splat_hip_camera_grad.h"

extern "C" int splat_camera_grad_abi_version(void) { return SPLAT_CAMERA_GRAD_ABI_VERSION; }

namespace {

constexpr int CAMG_BLOCK = 256, CAMG_PER_BLOCK = CAMG_BLOCK / 4;   // one quad per Gaussian: 64 Gaussians per workgroup
constexpr int CAMG_TD = 6;                                         // records in flight (the walk's TD for narrow records)
constexpr int FOLD_RANGES = 64, FOLD_BLOCK = FOLD_RANGES * 16;

struct CamGradArgs {
    int F, P, W, H, I, layout;
    int stride, dcol, nblk;
    long long cap;
    const float *pair;
    const int *goff;
    const DynTab *tab;
    const float *position, *cubic, *rotation;
    const float4 *rot_poly, *rot_fourier;
    const float *scaling, *extr, *intr;
    long long extr_fs, intr_fs;
    float *partials;
};

int64_t partial_rows(int F, int P) { return (int64_t)F * ((P + CAMG_PER_BLOCK - 1) / CAMG_PER_BLOCK); }

// grid (workgroups of 64 Gaussians, frame).  Lane j of a quad: lanes 0 and 1 load the record's first two 16-byte chunks (ux uy
// ga gb | gc ..), lane 2 the depth column; the quad re-evaluates the frame's position / rotation (lane j = component j) and lane
// 0 runs the chain under the frame's camera, which is uniform over the workgroup.  A (frame, Gaussian) without records adds
// nothing -- its coordinates are not even read (they may be non-finite).
template <bool PERSP>
__global__ void __launch_bounds__(CAMG_BLOCK) cam_grad_kernel(const CamGradArgs A) {
    __shared__ float red[CAMG_BLOCK / WAVE][16];
    const int f = blockIdx.y;
    const int t = blockIdx.x * CAMG_BLOCK + threadIdx.x;
    const int n = t >> 2, j = t & 3;
    float cg[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) cg[k] = 0.f;
    int beg = 0, end = 0;
    if (n < A.P) {
        const int *goff = A.goff + (size_t)f * A.P;
        beg = n > 0 ? goff[n - 1] : 0;
        end = imin_(goff[n], (int)A.cap);
    }
    if (end > beg) {   // quad-uniform
        float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float sd = 0.f;
        const float *base = A.pair + (size_t)f * (size_t)A.cap * A.stride;
        const bool chunk = j < 2, dep = j == 2 && A.dcol >= 0;
        for (int r = beg; r < end; r += CAMG_TD) {
            float4 v[CAMG_TD];
            float w[CAMG_TD];
#pragma unroll
            for (int u = 0; u < CAMG_TD; ++u) {
                const float *rec = base + (size_t)imin_(r + u, end - 1) * A.stride;
                const bool in = r + u < end;
                v[u] = (in && chunk) ? *reinterpret_cast<const float4 *>(rec + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
                w[u] = (in && dep) ? rec[A.dcol] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < CAMG_TD; ++u) { s4.x += v[u].x; s4.y += v[u].y; s4.z += v[u].z; s4.w += v[u].w; sd += w[u]; }
        }
        const float ux = quad_bcast<0>(s4.x), uy = quad_bcast<0>(s4.y);
        const float g3[3] = {quad_bcast<0>(s4.z), quad_bcast<0>(s4.w), quad_bcast<1>(s4.x)};
        const float gd = quad_bcast<2>(sd);
        const int seg = A.tab[f].seg;
        const CubicAddr ca = cubic_addr(A.layout, A.P, A.I, seg);
        const DynStatic stc = dyn_static(n, j, A.position, A.rotation, A.rot_poly, A.rot_fourier, A.scaling);
        const DynFrame fr = dyn_frame_rows(n, j, ca, A.tab[f].d, A.tab[f].basis, stc, A.cubic);
        if (j == 0) {
            Cam cam;   // F == 1 reads frame 0's camera whatever the stride (f == 0)
            load_cam(PERSP ? A.intr + (size_t)f * (size_t)A.intr_fs : nullptr, A.extr + (size_t)f * (size_t)A.extr_fs, cam);
            float c3[6], ea[3], eb[3], et[3], Jm[4], cov[3];
            cov3d_pt(fr.scl, fr.q, c3);
            ewa_T<!PERSP>(cam, fr.pos, A.W, A.H, ea, eb, et, Jm);
            ewa_cov2d<!PERSP>(ea, eb, c3, cov);
            if constexpr (PERSP) project_persp_camgrad_pt(cam, fr.pos[0], fr.pos[1], fr.pos[2], ux, uy, gd, cg);
            else project_ortho_camgrad_pt(fr.pos[0], fr.pos[1], fr.pos[2], A.W, A.H, ux, uy, gd, cg);
            const float det = cov[0] * cov[2] - cov[1] * cov[1];
            if (det != 0.0f) {   // the walk's gate
                float dcx, dcy, dcz, g6[6], da[3], db[3];
                ewa_grad_cov_pt(ea, eb, cov, det, g3, dcx, dcy, dcz, g6);
                if constexpr (PERSP) {
                    float ge[3], dt[3];
                    ewa_grad_pos_persp_pt(cam, et, ea, eb, c3, dcx, dcy, dcz, ge, da, db, dt);
                    ewa_persp_camgrad_pt(cam, fr.pos, et, Jm, da, db, dt, cg);
                } else {
                    ewa_grad_rows_pt(ea, eb, c3, dcx, dcy, dcz, da, db);
                    ewa_ortho_camgrad_pt(A.W, A.H, da, db, cg);
                }
            }
        }
    }
    // every lane of the workgroup takes part: DPP sums inside the wave, the four waves through LDS in wave order
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int k = PERSP ? 0 : 4; k < 16; ++k) {
        const float s = wave_sum_to_lane63(cg[k]);
        if (lane == WAVE - 1) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int k = threadIdx.x;
        const float s = (PERSP || k >= 4) ? ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k] : 0.f;
        A.partials[((size_t)f * A.nblk + blockIdx.x) * 16 + k] = s;
    }
}

// one workgroup per frame: thread (range c, component k) sums the rows of its range of workgroups in workgroup order, in
// float64; component k's 64 range sums are added in range order.  A per-frame camera's part is ADDED into its output row, a
// shared camera's part goes to frame_sums for cam_grad_frames_kernel.
struct CamFoldArgs {
    int F, nblk;
    const float *partials;
    double *frame_sums;
    float *d_extr, *d_intr;
    int extr_shared, intr_shared;
};

__global__ void __launch_bounds__(FOLD_BLOCK) cam_grad_fold_kernel(const CamFoldArgs A) {
    __shared__ double sh[FOLD_RANGES][16];
    const int f = blockIdx.x, c = threadIdx.x >> 4, k = threadIdx.x & 15;
    const int per = (A.nblk + FOLD_RANGES - 1) / FOLD_RANGES;
    const int b0 = imin_(c * per, A.nblk), b1 = imin_(b0 + per, A.nblk);
    const float *src = A.partials + (size_t)f * A.nblk * 16 + k;
    double acc = 0.0;
    for (int b = b0; b < b1; ++b) acc += (double)src[(size_t)b * 16];
    sh[c][k] = acc;
    __syncthreads();
    if (threadIdx.x < 16) {
        double tot = 0.0;
        for (int r = 0; r < FOLD_RANGES; ++r) tot += sh[r][k];
        const bool is_intr = k < 4;
        float *out = is_intr ? A.d_intr : A.d_extr;
        if (out) {
            if (is_intr ? A.intr_shared : A.extr_shared) A.frame_sums[(size_t)f * 16 + k] = tot;
            else {
                float *o = is_intr ? out + (size_t)f * 4 + k : out + (size_t)f * 12 + (k - 4);
                *o = (float)((double)*o + tot);
            }
        }
    }
}

// a camera shared by the frames: the frames' sums in frame order, ADDED into the one row
__global__ void __launch_bounds__(64) cam_grad_frames_kernel(const CamFoldArgs A) {
    const int k = threadIdx.x;
    if (k >= 16) return;
    const bool is_intr = k < 4;
    float *out = is_intr ? A.d_intr : A.d_extr;
    if (!out || !(is_intr ? A.intr_shared : A.extr_shared)) return;
    double tot = 0.0;
    for (int f = 0; f < A.F; ++f) tot += A.frame_sums[(size_t)f * 16 + k];
    float *o = is_intr ? out + k : out + (k - 4);
    *o = (float)((double)*o + tot);
}

}  // namespace

extern "C" int64_t splat_camera_grad_partials_floats(int F, int P) {
    if (F < 1 || P < 1) return 0;
    return partial_rows(F, P) * 16 + (int64_t)F * 32;   // the workgroups' rows, then [F,16] float64 frame sums
}

extern "C" int splat_frames_camera_backward_dynamic(int F, int P, int I, int W, int H, int64_t capacity, int record_stride,
                                                    int depth_column, const float *pair_records, const int32_t *goff_incl,
                                                    const void *tab, const float *position, const float *cubic,
                                                    int cubic_layout, const float *rotation, const float *rot_poly,
                                                    const float *rot_fourier, const float *scaling, const splat_camera_t *cam,
                                                    float *partials, float *d_extr, float *d_intr, void *stream) {
    SPLAT_CHECK_ARG(cam && cam->extr, "null camera (cam and cam->extr are required)");
    SPLAT_CHECK_ARG(!cam->perspective || cam->intr, "the perspective camera needs intr");
    SPLAT_CHECK_ARG(cam->perspective || !d_intr, "d_intr belongs to the perspective camera (an orthographic camera has no intr)");
    SPLAT_CHECK_ARG(cam->extr_frame_stride >= 0 && cam->intr_frame_stride >= 0, "negative camera stride");
    SPLAT_CHECK_ARG(F <= 65535, "more than 65535 frames (the frame is the grid's y dimension)");
    SPLAT_CHECK_ARG(F >= 1 && P >= 1 && I >= 1 && W > 0 && H > 0 && capacity >= 1 && capacity <= 0x7fffffff, "bad sizes");
    SPLAT_CHECK_ARG(record_stride >= 8 && record_stride % 4 == 0, "record_stride must be a multiple of 4 floats, at least 8");
    SPLAT_CHECK_ARG(depth_column < record_stride, "depth_column outside the record");
    SPLAT_CHECK_ARG(cubic_layout == SPLAT_CUBIC_GAUSSIAN_MAJOR || cubic_layout == SPLAT_CUBIC_SEGMENT_MAJOR, "unknown cubic_layout");
    SPLAT_CHECK_ARG(partials && ((uintptr_t)partials & 7) == 0, "null / misaligned partials (8-byte aligned scratch of "
                                                                "splat_camera_grad_partials_floats floats)");
    SPLAT_CHECK_ARG(pair_records && goff_incl && tab && position && cubic && rotation && rot_poly && rot_fourier && scaling,
                    "null input pointer");
    if (!d_extr && !d_intr) return SPLAT_OK;
    CamGradArgs A;
    memset(&A, 0, sizeof(A));
    A.F = F; A.P = P; A.W = W; A.H = H; A.I = I; A.layout = cubic_layout;
    A.stride = record_stride; A.dcol = depth_column < 0 ? -1 : depth_column; A.cap = capacity;
    A.nblk = (P + CAMG_PER_BLOCK - 1) / CAMG_PER_BLOCK;
    A.pair = pair_records; A.goff = goff_incl; A.tab = (const DynTab *)tab;
    A.position = position; A.cubic = cubic; A.rotation = rotation; A.rot_poly = (const float4 *)rot_poly;
    A.rot_fourier = (const float4 *)rot_fourier; A.scaling = scaling;
    A.extr = cam->extr; A.intr = cam->perspective ? cam->intr : nullptr;
    A.extr_fs = F == 1 ? 0 : cam->extr_frame_stride;
    A.intr_fs = F == 1 ? 0 : cam->intr_frame_stride;
    A.partials = partials;
    CamFoldArgs B;
    memset(&B, 0, sizeof(B));
    B.F = F; B.nblk = A.nblk; B.partials = partials;
    B.frame_sums = reinterpret_cast<double *>(partials + partial_rows(F, P) * 16);
    B.d_extr = d_extr; B.d_intr = d_intr;
    B.extr_shared = F > 1 && cam->extr_frame_stride == 0;
    B.intr_shared = F > 1 && cam->intr_frame_stride == 0;
    hipStream_t hs = (hipStream_t)stream;
    const dim3 grid((unsigned)A.nblk, (unsigned)F), block(CAMG_BLOCK);
    if (cam->perspective) SPLAT_LAUNCH("cam_grad", cam_grad_kernel<true>, grid, block, 0, hs, A);
    else SPLAT_LAUNCH("cam_grad", cam_grad_kernel<false>, grid, block, 0, hs, A);
    SPLAT_POST_LAUNCH();
    SPLAT_LAUNCH("cam_grad_fold", cam_grad_fold_kernel, dim3((unsigned)F), dim3(FOLD_BLOCK), 0, hs, B);
    SPLAT_POST_LAUNCH();
    if ((d_extr && B.extr_shared) || (d_intr && B.intr_shared)) {
        SPLAT_LAUNCH("cam_grad_fold", cam_grad_frames_kernel, dim3(1), dim3(64), 0, hs, B);
        SPLAT_POST_LAUNCH();
    }
    return SPLAT_OK;
}
