/* Fifth extension of the C ABI of libsplat_hip.so: DENSE OPTICAL FLOW of the learned video (the reference's
 * get_pred_flows_gs, src/trainer_fragGS.py:777-821): the per-Gaussian flow attribute of a batch of frame pairs with its
 * gradient, the Middlebury colouring of a flow map on the device (util.flow_to_image, src/util.py:421-536) and the flow error
 * against a reference flow with its gradient.
 *
 * The core header is frozen at its ABI version and the four extension headers before this one at their own; these entry
 * points are compiled into the same library and carry a version of their own.  Handles, structs (splat_camera_t) and error
 * codes are the core header's.  None of these functions uses a float atomic: all of them run under
 * splat_set_deterministic(1) and give the same bits on every run.
 */
#ifndef SPLAT_HIP_FLOW_H
#define SPLAT_HIP_FLOW_H

#include "splat_hip_layers_cam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_FLOW_ABI_VERSION 1
int splat_flow_abi_version(void);

/* flow [F,P,2] = uv(position(tab2[f]), cam2 frame f) - uv(position(tab1[f]), cam1 frame f) in pixels, one launch for the F
 * pairs.  tab1 / tab2: F device entries of 64 bytes each (the frame table of the batched dynamic preprocess); position [P,3],
 * cubic in either layout (I segments).  The spline position is the arithmetic of splat_dynamic_positions_batch_forward (same
 * operation order, same bits).  cam1 / cam2: one camera or one per pair (frame f reads extr + f * extr_frame_stride, 12
 * floats, a stride of 0 or >= 12; intr + f * intr_frame_stride, fx fy cx cy, a stride of 0 or >= 4), orthographic or pinhole
 * (the pinhole reciprocal is 1 / (z + 1e-7)); cam->offsets is not read.  cam2 == NULL: cam1 at both times.  Every product and
 * sum of the projection is rounded once (no contraction), both times run the same instructions: a pair whose two entries name
 * the same time under the same camera gives exactly +0.0.  A culled projection (depth <= nearest, uv outside extent) gives
 * uv = 0 as in the reference, so a Gaussian culled at one time only gives -uv1 or uv2; zero_culled != 0 writes 0 when either
 * side is culled.  P == 0 or F == 0: SPLAT_OK without a launch. */
int splat_flow_attribute_batch(int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                               const float *cubic, int cubic_layout, const splat_camera_t *cam1, const splat_camera_t *cam2,
                               int W, int H, float nearest, float extent, int zero_culled, float *flow, splat_stream_t stream);

/* Backward of the above: g [F,P,2] = dL/dflow goes back through both projections (the cull decisions are the forward's, a
 * culled side contributes zero; the cameras are constants) into d_position [P,3] and d_cubic (the layout of cubic), either
 * may be NULL.  accumulate == 0 zero-fills both first (d_cubic: P * 4 * I * 3 floats), accumulate != 0 adds.  One lane owns a
 * Gaussian's rows and walks the pairs in the order tab1's entries name (entry i's pad[0] = 1 + the pair to visit i-th, 0 =
 * table order: dynamics' walk order), the coefficient sums of a segment staying in registers until the walk leaves it, for
 * each of the two times on its own: every sum has a fixed order. */
int splat_flow_attribute_batch_backward(int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                                        const float *cubic, int cubic_layout, const splat_camera_t *cam1,
                                        const splat_camera_t *cam2, int W, int H, float nearest, float extent,
                                        int zero_culled, const float *g, int accumulate, float *d_position, float *d_cubic,
                                        splat_stream_t stream);

/* bytes of the scratch of splat_flow_to_image and splat_flow_error (per-workgroup partials) for F maps of H x W */
size_t splat_flow_scratch_bytes(int F, int H, int W);

/* Middlebury colours of flow maps: flow [F,2,H,W] (u plane, v plane) -> out [F,H,W,3] bytes (r g b), util.flow_to_image.
 * clip_flow > 0: both components are clamped to [0, clip_flow] first (np.clip(flow, 0, clip_flow)); <= 0: no clipping.
 * scale_mode SPLAT_FLOW_SCALE_PER_FRAME: every map is divided by its own maximum radius (the reference called on one map);
 * _WHOLE_CLIP: by the maximum over all F maps (the reference called on a stack); _GIVEN: by rad_max_in (the only mode in which
 * a radius above 1 occurs: those pixels take the wheel colour * 0.75).  Two passes: the maximum radius (float32 sqrt(u*u +
 * v*v), every operation rounded once; per-workgroup partials in `scratch`, one fold) and the colouring.  rad_max_out [F]
 * (device, may be NULL) receives the radius every map was divided by before the + 1e-5 (float32).  u, v, the radius, the
 * angle and the wheel position are float32, the colour interpolation (1 - f) c0 + f c1 and 255 * col are float64, as numpy
 * evaluates the reference.  DEVIATION: a pixel with a non-finite component is left out of the maximum and coloured black
 * (0, 0, 0); the reference propagates NaN into every pixel's scale. */
#define SPLAT_FLOW_SCALE_PER_FRAME 0
#define SPLAT_FLOW_SCALE_WHOLE_CLIP 1
#define SPLAT_FLOW_SCALE_GIVEN 2
int splat_flow_to_image(int F, int H, int W, const float *flow, float clip_flow, int scale_mode, float rad_max_in,
                        float *rad_max_out, uint8_t *out, int bgr, void *scratch, size_t scratch_bytes, splat_stream_t stream);

/* Flow error per map: pred, gt [F,2,H,W], weight [F,H,W] or NULL (1 everywhere), du = pred_u - gt_u, dv likewise.
 * sums [F,3] DOUBLE (device): sum w (|du| + |dv|), sum w sqrt(du*du + dv*dv), sum w.  A workgroup sums 2048 pixels in float32
 * in a fixed tree (partials in `scratch`), one thread per sum folds a map's partials in float64 in ascending order.
 * grad [F,2,H,W] or NULL: scale * w * sign(d) / max(sum_f w, 1e-30) -- the gradient of scale * (weighted-mean L1 of the map),
 * sign(0) = 0; a map whose weights are all zero gives sums 0 and a zero gradient. */
int splat_flow_error(int F, int H, int W, const float *pred, const float *gt, const float *weight, float scale, double *sums,
                     float *grad, void *scratch, size_t scratch_bytes, splat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
