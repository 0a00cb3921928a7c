/* Sixth extension of the C ABI of libsplat_hip.so: WHERE A DENSE FLOW IS VALID.  The flow attribute of a batch of frame pairs
 * with the depth at the second time beside uv2 - uv1 (scene flow's third channel and the track depth), and one fused per-pixel
 * kernel that looks frame t2 up at p + flow(p) and decides: target outside the frame, pixel not covered, something nearer at the
 * target (the depth test of the sparse tracker, the reference's get_correspondences_and_occlusion_masks_for_pixels_core,
 * src/trainer_fragGS.py:1644-1677, on every pixel), forward and backward flow inconsistent (Sundaram et al.); with the planes
 * of frame t2 pulled back to frame t1 by the same lookup.
 *
 * The core header and the five extension headers before this one are frozen at their versions; these entry points are compiled
 * into the same library and carry a version of their own.  Handles, structs (splat_camera_t) and error codes are the core
 * header's.  None of these functions uses a float atomic: all run under splat_set_deterministic(1), the same bits on every run.
 */
#ifndef SPLAT_HIP_FLOW_OCC_H
#define SPLAT_HIP_FLOW_OCC_H

#include "splat_hip_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_FLOW_OCC_ABI_VERSION 1
int splat_flow_occ_abi_version(void);

/* splat_flow_attribute_batch with the depth: out [F,P,4] = (u2 - u1, v2 - v1, z2 - z1, z2) per pair and Gaussian, one 16-byte
 * store each; z = the depth of the projection that gives uv.  Tables, layouts, cameras (one or per pair, orthographic or
 * pinhole, cam2 == NULL: cam1 at both times), cull rules and zero_culled are splat_flow_attribute_batch's; channels 0 and 1 are
 * its bits on the same arguments.  A culled side has uv = 0 and z = 0 (the reference's project_point leaves them so), so a
 * Gaussian culled at the second time has z2 = 0; zero_culled != 0 writes four +0.0 when either side is culled.  Equal times
 * under one camera give exactly +0.0 in channels 0 .. 2.  out: 16-byte aligned.  P == 0 or F == 0: SPLAT_OK without a launch. */
int splat_flow_attribute_depth_batch(int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                                     const float *cubic, int cubic_layout, const splat_camera_t *cam1,
                                     const splat_camera_t *cam2, int W, int H, float nearest, float extent, int zero_culled,
                                     float *out, splat_stream_t stream);

/* Backward of the above: g [F,P,4] goes into d_position [P,3] and d_cubic (either may be NULL) under the contract of
 * splat_flow_attribute_batch_backward (the lane owns its rows, tab1's walk order, per-segment register sums, accumulate, no
 * float atomics).  The depth of side 1 receives -g[2], the depth of side 2 g[2] + g[3]; a culled side contributes zero.  With
 * g[..., 2:] == 0 the result has the bits of splat_flow_attribute_batch_backward on g[..., :2].  g: 16-byte aligned. */
int splat_flow_attribute_depth_batch_backward(int F, int P, int I, const void *tab1, const void *tab2, const float *position,
                                              const float *cubic, int cubic_layout, const splat_camera_t *cam1,
                                              const splat_camera_t *cam2, int W, int H, float nearest, float extent,
                                              int zero_culled, const float *g, int accumulate, float *d_position,
                                              float *d_cubic, splat_stream_t stream);

/* bytes of the scratch of splat_flow_occlusion (per-workgroup integer partials of `counts`) for F maps of H x W */
size_t splat_flow_occlusion_scratch_bytes(int F, int H, int W);

/* Per pixel p = (x, y) of frame t1 with (u, v) = flow(p): q = (float(x) + u, float(y) + v) is the PIXEL-INDEX coordinate in
 * frame t2 -- the renderer's uv carries the -0.5, pixel i's centre is index i, nothing is rescaled.
 *
 * in:  flow [F,2,H,W]; track_depth [F,H,W] (the composited z2, background 0) and surface [F,H,W] (the depth render of frame
 *      t2, background bg_depth), both or neither; coverage [F,H,W] or NULL; flow_back [F,2,H,W] (the flow t2 -> t1) or NULL;
 *      src [F,C,H,W] (any planes of frame t2), 1 <= C <= 8, or NULL (then C == 0).
 * out: mask [F,H,W] bytes; depth_gap [F,H,W] (needs surface), fb_sq [F,H,W] (needs flow_back), warped [F,C,H,W] (needs src),
 *      each may be NULL; counts [F,4] int (pixels per bit, in bit order) or NULL -- per-workgroup integer partials in `scratch`
 *      (needed only with counts) and one fold.
 *
 * B(plane, q): x0 = floorf(qx), x1 = min(x0 + 1, W - 1), fx = qx - x0, likewise in y,
 *      B = ((v00 (1 - fx)) + (v01 fx)) (1 - fy) + ((v10 (1 - fx)) + (v11 fx)) fy.
 * OUTSIDE:      not (0 <= qx <= W - 1 && 0 <= qy <= H - 1); a non-finite flow is OUTSIDE.  Nothing is sampled; depth_gap,
 *               fb_sq and warped are +0.0.
 * UNCOVERED:    coverage given and not (coverage >= min_coverage).
 * IN_FRONT:     something nearer sits at the target: s = B(surface, q), td = track_depth + (1 - coverage) * bg_depth (coverage
 *               given: both sides composited over the same background; else td = track_depth), depth_gap = td - s, the bit
 *               is depth_gap > depth_margin.
 * INCONSISTENT: (bu, bv) = B(flow_back, q), ru = u + bu, rv = v + bv, fb_sq = ru ru + rv rv, the bit is
 *               fb_sq > fb_alpha ((u u + v v) + (bu bu + bv bv)) + fb_beta.
 * IN_FRONT and INCONSISTENT are set only when neither OUTSIDE nor UNCOVERED is; depth_gap, fb_sq and warped are written
 * whenever not OUTSIDE.  Every operation is one float32 operation rounded once, in the order written.  F == 0: SPLAT_OK without
 * a launch. */
#define SPLAT_FLOW_OCC_OUTSIDE 1
#define SPLAT_FLOW_OCC_UNCOVERED 2
#define SPLAT_FLOW_OCC_IN_FRONT 4
#define SPLAT_FLOW_OCC_INCONSISTENT 8
int splat_flow_occlusion(int F, int H, int W, int C, const float *flow, const float *track_depth, const float *surface,
                         const float *coverage, const float *flow_back, const float *src, float bg_depth, float depth_margin,
                         float min_coverage, float fb_alpha, float fb_beta, uint8_t *mask, float *depth_gap, float *fb_sq,
                         float *warped, int *counts, void *scratch, size_t scratch_bytes, splat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
