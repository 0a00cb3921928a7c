/* Second extension of the C ABI of libsplat_hip.so: TRAINING a dynamic batch under the cameras of include/splat_hip_views.h.
 *
 * The core header is frozen at its ABI version and the views header at its own; the Gaussian-side backward of a frame batch
 * of dynamic Gaussians under cameras that differ per frame and under the pinhole camera lives here, is compiled into the
 * same library and carries a version of its own.  Handles, structs (splat_camera_t) and error codes are the core header's.
 */
#ifndef SPLAT_HIP_VIEWS_GRAD_H
#define SPLAT_HIP_VIEWS_GRAD_H

#include "splat_hip_views.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_VIEWS_GRAD_ABI_VERSION 1
int splat_views_grad_abi_version(void);

/* The Gaussian-side backward of a frame batch of dynamic Gaussians whose forward was
 * splat_frame_preprocess_forward_batch_cam: every argument but `cam` is the one of the core header's
 * splat_frames_gauss_backward_dynamic / _sets / _sources (pair records of the tile backward, goff, radius, the frame table,
 * the parameters; gradients ADDED into d_*).  cam->perspective == 0 with ONE camera (extr_frame_stride == 0, or F == 1) calls
 * that entry point itself and gives its bits.  Cameras that differ per frame (frame f reads extr + f * extr_frame_stride, 12
 * floats) and the pinhole camera (intr + f * intr_frame_stride: fx fy cx cy; a stride of 0 = one for all frames) run
 * instantiations of their own: every frame's records go back through that frame's projection and EWA under that frame's
 * camera, and under the pinhole camera the position gradient includes the term through the conic.  The cameras are constants:
 * no gradient with respect to extr / intr.  No float atomics: two runs give the same bits.  cam->offsets is not read.
 * NULL cam / cam->extr, a perspective camera without intr and a negative stride are SPLAT_E_ARG. */
int splat_frames_gauss_backward_dynamic_cam(int F, int P, int I, int C, int W, int H, int64_t capacity, int want_abs,
                                            const float *pair_records, const int32_t *goff_incl, const int32_t *radius,
                                            const void *tab, const float *position, const float *cubic, int cubic_layout,
                                            const float *rotation, const float *rot_poly, const float *rot_fourier,
                                            const float *opacity, const float *scaling, const splat_camera_t *cam,
                                            float *d_position, float *d_cubic, float *d_rotation, float *d_opacity,
                                            float *d_scaling, float *d_feature, float *tap, float *abs_tap,
                                            int32_t *radii_max, splat_stream_t stream);
int splat_frames_gauss_backward_dynamic_sets_cam(int F, int P, int I, int C, int W, int H, int64_t capacity,
                                                 const float *pair_records, const int32_t *goff_incl, const int32_t *radius,
                                                 const void *tab, const float *position, const float *cubic, int cubic_layout,
                                                 const float *rotation, const float *rot_poly, const float *rot_fourier,
                                                 const float *opacity, const float *scaling, const splat_camera_t *cam,
                                                 float *d_position, float *d_cubic, float *d_rotation, float *d_opacity,
                                                 float *d_scaling, const int32_t *set_c0, const int32_t *set_cn,
                                                 float *const *set_dfeature, const int32_t *set_stride, int depth_channel,
                                                 float *tap, float *abs_tap, int32_t *radii_max, splat_stream_t stream);
int splat_frames_gauss_backward_dynamic_sources_cam(int F, int P, int I, int C, int W, int H, int64_t capacity,
                                                    const float *pair_records, const int32_t *goff_incl,
                                                    const int32_t *radius, const void *tab, const float *position,
                                                    const float *cubic, int cubic_layout, const float *rotation,
                                                    const float *rot_poly, const float *rot_fourier, const float *opacity,
                                                    const float *scaling, const splat_camera_t *cam, float *d_position,
                                                    float *d_cubic, float *d_rotation, float *d_opacity, float *d_scaling,
                                                    int nsrc, const splat_feature_source_t *src, int depth_channel,
                                                    float *tap, float *abs_tap, int32_t *radii_max, splat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
