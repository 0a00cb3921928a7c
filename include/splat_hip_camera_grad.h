/* Third extension of the C ABI of libsplat_hip.so: the CAMERA gradients of a dynamic frame batch.
 *
 * The core header and the two extensions before this one (splat_hip_views.h, splat_hip_views_grad.h) are frozen at their ABI
 * versions.  Their Gaussian-side backward treats the cameras of a batch as constants; the entry point here gives dL/dextr (12
 * numbers per frame: the rows of [R|T]) and, under the pinhole camera, dL/dintr (fx fy cx cy per frame) of the same pair
 * records.  Compiled into the same library, a version of its own.  Handles, structs (splat_camera_t) and error codes are the
 * core header's.
 *
 * Per (frame f, Gaussian g) that owns records in f (goff_incl[f][g] > goff_incl[f][g - 1]) the kernel sums the records'
 * columns 0 .. 4 (dL/du, dL/dv, dL/dconic a b c) and the depth column, re-evaluates the frame's position and rotation as the
 * Gaussian-side walk does and forms the contribution under frame f's camera (extr + f * extr_frame_stride, intr + f *
 * intr_frame_stride; a stride of 0 = one camera).  A pair without records contributes nothing -- not 0 times its coordinates,
 * which may be non-finite.  With p = (x, y, z, 1) and da, db = dL/d(rows of T = J R) from dL/dcov2d, where det(cov2d) != 0:
 *   pinhole       the arithmetic of the per-operator project_point / ewa_project backward (the reference's dL_dintr / dL_dextr);
 *   orthographic  d e[k]     = p[k] dL/du W/2 + (k < 3) W/2 da[k]
 *                 d e[4 + k] = p[k] dL/dv H/2 + (k < 3) H/2 db[k]
 *                 d e[8 + k] = p[k] dL/ddepth.
 * Not differentiated: the cull / near / extent decisions and the radius.
 *
 * No float atomics; two runs give the same bits.  Launch 1 ("cam_grad"): one quad per (Gaussian, frame); DPP sums inside the
 * wave, the four waves of a workgroup through LDS in wave order, one row of 16 floats (intr 0 .. 3, extr 4 .. 15) per workgroup
 * into `partials`.  Launch 2 ("cam_grad_fold"): per frame the rows are summed in float64 in a fixed order (64 consecutive
 * ranges of workgroups, each in workgroup order, then the ranges in order) and ADDED into the outputs; a camera whose stride
 * is 0 (F > 1) receives the sum of the frames, in frame order, from a third small launch of the same name.
 */
#ifndef SPLAT_HIP_CAMERA_GRAD_H
#define SPLAT_HIP_CAMERA_GRAD_H

#include "splat_hip_views_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_CAMERA_GRAD_ABI_VERSION 1
int splat_camera_grad_abi_version(void);

/* floats of the `partials` scratch of splat_frames_camera_backward_dynamic for F frames of P Gaussians (the library owns no
 * buffer: the caller allocates it, 8-byte aligned); 0 for F < 1 or P < 1 */
int64_t splat_camera_grad_partials_floats(int F, int P);

/* pair_records [F, capacity, record_stride] floats (record_stride a multiple of 4, >= 8: plain and SETS records alike),
 * depth_column = the record's column that holds dL/ddepth (SETS records: 12 + depth channel) or -1: no depth gradient.
 * goff_incl, tab, position .. scaling, cubic_layout: as splat_frames_gauss_backward_dynamic_cam.  d_extr [F,12] floats, or
 * [12] when cam->extr_frame_stride == 0; d_intr [F,4] or [4] (pinhole only); both are ADDED to; either may be NULL, both NULL
 * returns SPLAT_OK without a launch.  SPLAT_E_ARG in front of any HIP call: NULL cam / cam->extr / partials, a perspective
 * camera without intr, d_intr with an orthographic camera, a negative stride, depth_column >= record_stride, bad sizes.
 * cam->offsets is not read. */
int splat_frames_camera_backward_dynamic(int F, int P, int I, int W, int H, int64_t capacity, int record_stride,
                                         int depth_column, const float *pair_records, const int32_t *goff_incl,
                                         const void *tab, const float *position, const float *cubic, int cubic_layout,
                                         const float *rotation, const float *rot_poly, const float *rot_fourier,
                                         const float *scaling, const splat_camera_t *cam, float *partials, float *d_extr,
                                         float *d_intr, splat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
