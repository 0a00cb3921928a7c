/* Fourth extension of the C ABI of libsplat_hip.so: LAYERED scenes (layer editing, feature lifting) under the cameras of
 * include/splat_hip_views.h.
 *
 * The core header is frozen at its ABI version and the three extension headers before this one at their own; the preprocess of
 * one layer of a layered scene under cameras that differ per frame and under the pinhole camera lives here, is compiled into
 * the same library and carries a version of its own.  Handles, structs (splat_camera_t) and error codes are the core header's.
 * Forward only.
 */
#ifndef SPLAT_HIP_LAYERS_CAM_H
#define SPLAT_HIP_LAYERS_CAM_H

#include "splat_hip_views.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_LAYERS_CAM_ABI_VERSION 1
int splat_layers_cam_abi_version(void);

/* One layer of a batch of Q instances under any camera: every argument but `cam` is the one of the core header's
 * splat_frame_preprocess_layer_batch (quad s evaluates source Gaussian src[s] -- src == NULL: s -- at the layer's own frame
 * table `tab` and writes row q0 + s of uv / depth / conic / radius [F,Q,..] and opa_t [Q]; the similarity transform
 * ((p - c) * scale + c) + delta with centroid / delta [F,3], every step rounded to float32, in world space, before the
 * projection; scale_splats multiplies the activated scale).  cam->perspective == 0 with ONE camera (extr_frame_stride == 0, or
 * F == 1) calls that entry point itself and gives its bits.  Cameras that differ per frame (frame f reads extr + f *
 * extr_frame_stride, 12 floats; a stride of 0 or >= 12) and the pinhole camera (intr + f * intr_frame_stride: fx fy cx cy; a
 * stride of 0 = one for all frames, or >= 4) run a kernel of their own: `depth` is the instance's depth under its frame's
 * camera.  The centroids (splat_layer_centroids) do not depend on the camera.  No atomics: two runs give the same bits.  A
 * source id outside the model writes nothing.  cam->offsets is not read.  NULL cam / cam->extr, a perspective camera without
 * intr and a stride that is negative or shorter than a row are SPLAT_E_ARG. */
int splat_frame_preprocess_layer_batch_cam(int F, int P, int S, int Q, int q0, int I, const void *tab, const int32_t *src,
                                           const float *position, const float *cubic, int cubic_layout, const float *rotation,
                                           const float *rot_poly, const float *rot_fourier, const float *opacity,
                                           const float *scaling, const splat_camera_t *cam, int W, int H, float nearest,
                                           float extent, const float *centroid, const float *delta, float scale,
                                           int scale_splats, float *uv, float *depth, float *conic, int32_t *radius,
                                           float *opa_t, splat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
