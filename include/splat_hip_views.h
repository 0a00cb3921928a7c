/* Extension of the C ABI of libsplat_hip.so: viewing a learned video from elsewhere (novel-view orbits, stereo clips).
 *
 * The core header include/splat_hip.h is frozen at its ABI version; entry points added after it live here, are compiled into
 * the same library and carry a version of their own.  Handles (splat_stream_t), structs (splat_camera_t) and the error
 * codes are the core header's.  Forward only: none of these functions has a backward.
 */
#ifndef SPLAT_HIP_VIEWS_H
#define SPLAT_HIP_VIEWS_H

#include "splat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_VIEWS_ABI_VERSION 1
int splat_views_abi_version(void);

/* The batched preprocess of dynamic Gaussians under any camera: every argument but `cam` is the one of the core header's
 * batched dynamic preprocess (tab = F device entries of 64 bytes, cubic in either layout, outputs [F,P,..], opa_t [P]).
 * cam->perspective == 0 with ONE camera (extr_frame_stride == 0, or F == 1) launches that entry point's own kernel and
 * gives its bits; cameras that differ per frame (frame f reads extr + f * extr_frame_stride, 12 floats) and the pinhole camera
 * (intr + f * intr_frame_stride: fx fy cx cy) run a kernel of their own.  cam->offsets is not read. */
int splat_frame_preprocess_forward_batch_cam(int F, int P, int I, const void *tab, const float *position, const float *cubic,
                                             int cubic_layout, const float *rotation, const float *rot_poly,
                                             const float *rot_fourier, const float *opacity, const float *scaling,
                                             const splat_camera_t *cam, int W, int H, float nearest, float extent, float *uv,
                                             float *depth, float *conic, int32_t *radius, float *opa_t,
                                             splat_stream_t stream);

/* Display-ready frames: a, b = dense float images [F,3,H,W] (b may be NULL), out = [F,H,W,3] bytes.
 * Without b: v = min(max(x, 0), 1) with NaN -> 0, byte = (uint8)(v * 255.0f), truncated.
 * With b (a = left eye, b = right eye, both clamped as above): mix_host = 18 HOST floats, a 3 x 6 matrix m over
 * (left r g b, right r g b), read during the call; o_c = ((((m[c][0] l_r + m[c][1] l_g) + m[c][2] l_b) + m[c][3] r_r) +
 * m[c][4] r_g) + m[c][5] r_b in float32, every product and sum rounded once; byte = (uint8) min(max(o_c * 255.0f, 0), 255).
 * mix_host is ignored without b. */
int splat_frames_present(int F, int H, int W, const float *a, const float *b, const float *mix_host, uint8_t *out,
                         splat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
