// Gaussian-side backward of a frame batch of dynamic Gaussians under cameras per frame and the pinhole camera
// (include/splat_hip_views_grad.h): the CAM = 1 / CAM = 2 instantiations of frames_gauss_bwd_dynamic_kernel (gauss_dyn_bwd.h)
// and their three entry points.  One orthographic camera is handed to the core entry point (preprocess.hip: CAM = 0, its
// bits).  A translation unit of its own: the kernel is slow to compile and these are twice the instantiations CAM = 0 has.
#include "gauss_dyn_bwd.h"
#include "../../include/splat_hip_views_grad.h"

extern "C" size_t splat_blend_pair_stride(int C, int want_abs, int has_bias);
extern "C" size_t splat_blend_sets_pair_stride(int C);

extern "C" int splat_views_grad_abi_version(void) { return SPLAT_VIEWS_GRAD_ABI_VERSION; }

namespace {

// the forward's rule (splat_frame_preprocess_forward_batch_cam): one orthographic camera is the core entry point's
bool one_ortho_camera(const splat_camera_t *cam, int F) {
    return !cam->perspective && (cam->extr_frame_stride == 0 || F == 1);
}

int check_camera(const splat_camera_t *cam) {
    SPLAT_CHECK_ARG(cam && cam->extr, "null camera (cam and cam->extr are required)");
    SPLAT_CHECK_ARG(!cam->perspective || cam->intr, "the perspective camera needs intr");
    SPLAT_CHECK_ARG(cam->extr_frame_stride >= 0 && cam->intr_frame_stride >= 0, "negative camera stride");
    return SPLAT_OK;
}

// the arguments every entry point shares (the checks of the core twins)
int fill_args(GaussDynArgs &A, int F, int P, int I, int C, int cmax, int W, int H, int64_t capacity, const float *pair_records,
              const int32_t *goff_incl, const int32_t *radius, const void *tab, const float *position, const float *cubic,
              int cubic_layout, const float *rotation, const float *rot_poly, const float *rot_fourier, const float *opacity,
              const float *scaling, const splat_camera_t *cam, float *d_position, float *d_cubic, float *d_rotation,
              float *d_opacity, float *d_scaling, float *tap, float *abs_tap, int32_t *radii_max) {
    SPLAT_CHECK_ARG(F >= 1 && P >= 1 && I >= 1 && C >= 1 && C <= cmax && W > 0 && H > 0 && capacity >= 1, "bad sizes");
    SPLAT_CHECK_ARG(cubic_layout == SPLAT_CUBIC_GAUSSIAN_MAJOR || cubic_layout == SPLAT_CUBIC_SEGMENT_MAJOR, "unknown cubic_layout");
    SPLAT_CHECK_ARG(pair_records && goff_incl && tab && position && cubic && rotation && rot_poly && rot_fourier && opacity && scaling,
                    "null input pointer");
    SPLAT_CHECK_ARG(!radii_max || radius, "radii_max needs the per-frame radius");
    memset(&A, 0, sizeof(A));
    A.F = F; A.P = P; A.W = W; A.H = H; A.I = I; A.layout = cubic_layout; A.C = C; A.cn = C; A.cap = capacity;
    A.pair = pair_records; A.goff = goff_incl; A.radius = radius; A.tab = (const DynTab *)tab;
    A.position = position; A.cubic = cubic; A.rotation = rotation; A.rot_poly = (const float4 *)rot_poly;
    A.rot_fourier = (const float4 *)rot_fourier; A.opacity = opacity; A.scaling = scaling;
    A.extr = cam->extr; A.intr = cam->perspective ? cam->intr : nullptr;
    // F == 1 reads frame 0's camera whatever the stride
    A.extr_fs = F == 1 ? 0 : cam->extr_frame_stride;
    A.intr_fs = F == 1 ? 0 : cam->intr_frame_stride;
    A.d_position = d_position; A.d_cubic = d_cubic; A.d_rotation = d_rotation; A.d_opacity = d_opacity; A.d_scaling = d_scaling;
    A.tap = tap; A.abs_tap = abs_tap; A.radii_max = radii_max;
    A.depth_channel = -1;
    return SPLAT_OK;
}

}  // namespace

extern "C" int splat_frames_gauss_backward_dynamic_cam(int F, int P, int I, int C, int W, int H, int64_t capacity, int want_abs,
                                                       const float *pair_records, const int32_t *goff_incl,
                                                       const int32_t *radius, const void *tab, const float *position,
                                                       const float *cubic, int cubic_layout, const float *rotation,
                                                       const float *rot_poly, const float *rot_fourier, const float *opacity,
                                                       const float *scaling, const splat_camera_t *cam, float *d_position,
                                                       float *d_cubic, float *d_rotation, float *d_opacity, float *d_scaling,
                                                       float *d_feature, float *tap, float *abs_tap, int32_t *radii_max,
                                                       void *stream) {
    if (const int rc = check_camera(cam)) return rc;
    if (one_ortho_camera(cam, F))
        return splat_frames_gauss_backward_dynamic(F, P, I, C, W, H, capacity, want_abs, pair_records, goff_incl, radius, tab,
                                                   position, cubic, cubic_layout, rotation, rot_poly, rot_fourier, opacity, scaling,
                                                   cam->extr, d_position, d_cubic, d_rotation, d_opacity, d_scaling, d_feature, tap,
                                                   abs_tap, radii_max, stream);
    GaussDynArgs A;
    if (const int rc = fill_args(A, F, P, I, C, 32, W, H, capacity, pair_records, goff_incl, radius, tab, position, cubic,
                                 cubic_layout, rotation, rot_poly, rot_fourier, opacity, scaling, cam, d_position, d_cubic,
                                 d_rotation, d_opacity, d_scaling, tap, abs_tap, radii_max))
        return rc;
    SPLAT_CHECK_ARG(!abs_tap || want_abs, "abs_tap needs records with the abs sums");
    A.d_feature = d_feature;
    const int ncp = (int)splat_blend_pair_stride(C, want_abs, 0);
    hipStream_t hs = (hipStream_t)stream;
    if (cam->perspective) return want_abs ? launch_gauss_bwd_dynamic<true, 2>(A, ncp, hs) : launch_gauss_bwd_dynamic<false, 2>(A, ncp, hs);
    return want_abs ? launch_gauss_bwd_dynamic<true, 1>(A, ncp, hs) : launch_gauss_bwd_dynamic<false, 1>(A, ncp, hs);
}

extern "C" int splat_frames_gauss_backward_dynamic_sets_cam(int F, int P, int I, int C, int W, int H, int64_t capacity,
                                                            const float *pair_records, const int32_t *goff_incl,
                                                            const int32_t *radius, const void *tab, const float *position,
                                                            const float *cubic, int cubic_layout, const float *rotation,
                                                            const float *rot_poly, const float *rot_fourier,
                                                            const float *opacity, const float *scaling,
                                                            const splat_camera_t *cam, float *d_position, float *d_cubic,
                                                            float *d_rotation, float *d_opacity, float *d_scaling,
                                                            const int32_t *set_c0, const int32_t *set_cn,
                                                            float *const *set_dfeature, const int32_t *set_stride,
                                                            int depth_channel, float *tap, float *abs_tap, int32_t *radii_max,
                                                            void *stream) {
    if (const int rc = check_camera(cam)) return rc;
    if (one_ortho_camera(cam, F))
        return splat_frames_gauss_backward_dynamic_sets(F, P, I, C, W, H, capacity, pair_records, goff_incl, radius, tab, position,
                                                        cubic, cubic_layout, rotation, rot_poly, rot_fourier, opacity, scaling,
                                                        cam->extr, d_position, d_cubic, d_rotation, d_opacity, d_scaling, set_c0,
                                                        set_cn, set_dfeature, set_stride, depth_channel, tap, abs_tap, radii_max,
                                                        stream);
    GaussDynArgs A;
    if (const int rc = fill_args(A, F, P, I, C, 28, W, H, capacity, pair_records, goff_incl, radius, tab, position, cubic,
                                 cubic_layout, rotation, rot_poly, rot_fourier, opacity, scaling, cam, d_position, d_cubic,
                                 d_rotation, d_opacity, d_scaling, tap, abs_tap, radii_max))
        return rc;
    SPLAT_CHECK_ARG(set_c0 && set_cn && set_dfeature && set_stride, "null set table");
    SPLAT_CHECK_ARG(depth_channel < C, "depth_channel outside the row");
    A.depth_channel = depth_channel;
    A.nsrc = 3;
    for (int g = 0; g < 3; ++g) {
        A.sc0[g] = set_c0[g]; A.scn[g] = set_cn[g]; A.sstride[g] = set_stride[g]; A.sdf[g] = set_dfeature[g];
        SPLAT_CHECK_ARG(set_cn[g] == 0 || !set_dfeature[g] || set_stride[g] >= set_cn[g], "feature stride below the set width");
    }
    const int ncp = (int)splat_blend_sets_pair_stride(C);
    return cam->perspective ? launch_gauss_bwd_dynamic_sets<2>(A, ncp, (hipStream_t)stream)
                            : launch_gauss_bwd_dynamic_sets<1>(A, ncp, (hipStream_t)stream);
}

extern "C" int splat_frames_gauss_backward_dynamic_sources_cam(int F, int P, int I, int C, int W, int H, int64_t capacity,
                                                               const float *pair_records, const int32_t *goff_incl,
                                                               const int32_t *radius, const void *tab, const float *position,
                                                               const float *cubic, int cubic_layout, const float *rotation,
                                                               const float *rot_poly, const float *rot_fourier,
                                                               const float *opacity, const float *scaling,
                                                               const splat_camera_t *cam, float *d_position, float *d_cubic,
                                                               float *d_rotation, float *d_opacity, float *d_scaling, int nsrc,
                                                               const splat_feature_source_t *src, int depth_channel, float *tap,
                                                               float *abs_tap, int32_t *radii_max, void *stream) {
    if (const int rc = check_camera(cam)) return rc;
    if (one_ortho_camera(cam, F))
        return splat_frames_gauss_backward_dynamic_sources(F, P, I, C, W, H, capacity, pair_records, goff_incl, radius, tab,
                                                           position, cubic, cubic_layout, rotation, rot_poly, rot_fourier, opacity,
                                                           scaling, cam->extr, d_position, d_cubic, d_rotation, d_opacity, d_scaling,
                                                           nsrc, src, depth_channel, tap, abs_tap, radii_max, stream);
    GaussDynArgs A;
    if (const int rc = fill_args(A, F, P, I, C, 28, W, H, capacity, pair_records, goff_incl, radius, tab, position, cubic,
                                 cubic_layout, rotation, rot_poly, rot_fourier, opacity, scaling, cam, d_position, d_cubic,
                                 d_rotation, d_opacity, d_scaling, tap, abs_tap, radii_max))
        return rc;
    SPLAT_CHECK_ARG(src && nsrc >= 0 && nsrc <= SPLAT_MAX_SOURCES, "null / oversized source table");
    SPLAT_CHECK_ARG(depth_channel < C, "depth_channel outside the row");
    A.depth_channel = depth_channel;
    A.nsrc = nsrc;
    for (int g = 0; g < nsrc; ++g) {   // (the table of splat_frames_gauss_backward_dynamic_sources)
        SPLAT_CHECK_ARG(src[g].cn >= 0 && src[g].c0 >= 0 && src[g].c0 + src[g].cn <= C, "source outside the row");
        SPLAT_CHECK_ARG(src[g].frame_stride == 0 || !src[g].d_feature || src[g].frame_stride >= (int64_t)P * src[g].cn,
                        "frame stride of a per-frame source below P * cn");
        A.sc0[g] = src[g].c0; A.scn[g] = src[g].cn; A.sstride[g] = src[g].cn; A.sdf[g] = src[g].d_feature;
        A.sfs[g] = src[g].d_feature ? src[g].frame_stride : 0;
        if (A.sfs[g] != 0) ++A.npf;
        const int k0 = SETS_NG + src[g].c0, k1 = k0 + src[g].cn - 1;
        A.spfq[g] = (src[g].cn >= 1 && k0 / 4 == k1 / 4) ? k0 / 4 : -1;
    }
    const int ncp = (int)splat_blend_sets_pair_stride(C);
    return cam->perspective ? launch_gauss_bwd_dynamic_sets<2>(A, ncp, (hipStream_t)stream)
                            : launch_gauss_bwd_dynamic_sets<1>(A, ncp, (hipStream_t)stream);
}
