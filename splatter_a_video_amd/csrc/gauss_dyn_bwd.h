// Gaussian-side backward of a frame batch of DYNAMIC Gaussians: the per-frame evaluation helpers, the kernel and its
// launchers.  A header because two translation units instantiate the kernel: preprocess.hip the one orthographic camera
// (CAM = 0), gauss_dyn_cam.hip the cameras per frame and the pinhole camera (CAM = 1, 2: twice as many instantiations as
// CAM = 0 has, compiled beside preprocess.hip instead of behind it).
#pragma once
#include "common.h"
#include "pointwise_dev.h"
#include "dynamics_dev.h"

namespace {

struct DynFrame {
    float pos[3], q[4], scl[3];  // per-frame position, normalised rotation, activated scale
    float qraw[4], nrm;          // un-normalised rotation and its norm (backward)
};

__device__ __forceinline__ DynFrame dyn_frame(int n, int j, const CubicAddr &ca, float d, const DynBasis &b,
                                              const float *position, const float *cubic, const float *rotation,
                                              const float4 *rot_poly, const float4 *rot_fourier, const float *scaling) {
    float pj = 0.f, sj = 0.f;
    if (j < 3) {
        const float *c = cubic + ca.seg_off + (size_t)n * ca.stride_n + j;
        const size_t row = ca.stride_k;
        const float c0 = c[0], c1 = c[row], c2 = c[2 * row], c3 = c[3 * row];
        float p = c3 + c2 * d;
        p = p + c1 * (d * d);
        p = p + c0 * (d * d * d);
        pj = p + position[(size_t)n * 3 + j];
        sj = expf(scaling[(size_t)n * 3 + j]);
    }
    const float qj = quat_component(n, j, b, rotation, rot_poly, rot_fourier);
    const float nr = sqrtf(quad_sum(qj * qj));
    const float qn = qj / fmaxf(nr, 1e-12f);  // F.normalize: x / max(|x|, eps)
    DynFrame f;
    f.pos[0] = quad_bcast<0>(pj); f.pos[1] = quad_bcast<1>(pj); f.pos[2] = quad_bcast<2>(pj);
    f.scl[0] = quad_bcast<0>(sj); f.scl[1] = quad_bcast<1>(sj); f.scl[2] = quad_bcast<2>(sj);
    f.q[0] = quad_bcast<0>(qn); f.q[1] = quad_bcast<1>(qn); f.q[2] = quad_bcast<2>(qn); f.q[3] = quad_bcast<3>(qn);
    f.qraw[0] = quad_bcast<0>(qj); f.qraw[1] = quad_bcast<1>(qj); f.qraw[2] = quad_bcast<2>(qj); f.qraw[3] = quad_bcast<3>(qj);
    f.nrm = nr;
    return f;
}

// frame-loop form: position row, log-scale and the rotation table rows stay in registers across the frames
struct DynStatic {
    float pos_j, scl_j;  // position[n][j], exp(scaling[n][j])  (j < 3)
    QuatRows rows;
};
__device__ __forceinline__ DynStatic dyn_static(int n, int j, const float *position, const float *rotation,
                                                const float4 *rot_poly, const float4 *rot_fourier, const float *scaling) {
    DynStatic s;
    s.pos_j = j < 3 ? position[(size_t)n * 3 + j] : 0.f;
    s.scl_j = j < 3 ? expf(scaling[(size_t)n * 3 + j]) : 0.f;
    s.rows = load_quat_rows(n, j, rotation, rot_poly, rot_fourier);
    return s;
}
__device__ __forceinline__ DynFrame dyn_frame_rows(int n, int j, const CubicAddr &ca, float d, const float *basis12,
                                                   const DynStatic &st, const float *cubic) {
    float pj = 0.f;
    if (j < 3) {
        const float *c = cubic + ca.seg_off + (size_t)n * ca.stride_n + j;
        const size_t row = ca.stride_k;
        const float c0 = c[0], c1 = c[row], c2 = c[2 * row], c3 = c[3 * row];
        float p = c3 + c2 * d;
        p = p + c1 * (d * d);
        p = p + c0 * (d * d * d);
        pj = p + st.pos_j;
    }
    const float qj = quat_component_rows(st.rows, j, basis12[j], basis12[4 + j], basis12[8 + j]);
    const float nr = sqrtf(quad_sum(qj * qj));
    const float qn = qj / fmaxf(nr, 1e-12f);
    DynFrame f;
    f.pos[0] = quad_bcast<0>(pj); f.pos[1] = quad_bcast<1>(pj); f.pos[2] = quad_bcast<2>(pj);
    f.scl[0] = quad_bcast<0>(st.scl_j); f.scl[1] = quad_bcast<1>(st.scl_j); f.scl[2] = quad_bcast<2>(st.scl_j);
    f.q[0] = quad_bcast<0>(qn); f.q[1] = quad_bcast<1>(qn); f.q[2] = quad_bcast<2>(qn); f.q[3] = quad_bcast<3>(qn);
    f.qraw[0] = quad_bcast<0>(qj); f.qraw[1] = quad_bcast<1>(qj); f.qraw[2] = quad_bcast<2>(qj); f.qraw[3] = quad_bcast<3>(qj);
    f.nrm = nr;
    return f;
}

// Backward: one quad per Gaussian walks ALL frames: per frame it sums the Gaussian's pair records (lane `sub` owns the
// record chunks sub, sub + 4, ..), re-evaluates the frame's position / rotation (dyn_frame), runs projection + EWA +
// cov3d backward and chains through the activations -- scale = exp, rotation = normalize(raw + detached sums), opacity =
// sigmoid, position = base + cubic segment.  Everything accumulates in registers; the spline segment's four coefficient
// rows are flushed when the walk leaves the segment (frames of a batch are time-ordered: a handful of flushes).
// 168 registers, no scratch (4: 128 registers and 156 bytes of scratch per lane -- 62 vs 54 us per frame for the three-set
// records at c2, round 4)
//
// CAM (the meaning of frames_gauss_bwd_static_kernel's): 0 = ONE orthographic camera, read once, uniform.  1 = orthographic
// cameras that differ from frame to frame, 2 = the pinhole camera: in the four-frame trip lane k loads frame f + k's camera
// (extr + (f + k) * extr_fs, intr + (f + k) * intr_fs; a stride of 0 = one camera for all frames) at the top of the trip,
// ahead of the slot ranges and the records, as frame_preprocess_fwd_batch_cam_kernel does, and runs the chain for its own
// frame under it.  Under CAM = 2 the Jacobian depends on the frame's position: the position gradient gains the term through
// the conic (ewa_grad_pos_persp_pt) and uv / depth go back through project_persp_grad_pt.  A per-lane camera is 12 (16)
// vector registers where CAM = 0 holds scalars: CAM > 0 is bounded for two waves per SIMD instead of three, and CAM = 0 is
// left as it was.  No LDS, no atomics in any mode.
constexpr int GAUSS_DYN_MINW = 3, GAUSS_DYN_MINW_CAM = 2;
struct GaussDynArgs {
    int F, P, W, H, I, layout;
    int C, cn;
    long long cap;
    const float *pair;
    const int *goff;
    const int *radius;
    const DynTab *tab;
    const float *position, *cubic, *rotation;
    const float4 *rot_poly, *rot_fourier;
    const float *opacity, *scaling, *extr;
    float *d_position, *d_cubic, *d_rotation, *d_opacity, *d_scaling, *d_feature;  // d_cubic / d_* are ADDED to
    float *tap, *abs_tap;
    int *radii_max;
    // SETS records (blend_bwd_sets_kernel): see GaussBwdArgs
    // (sources: nsrc entries; sfs[g] != 0 = per-frame source whose gradient is ADDED per frame at sdf[g] + f * sfs[g]; npf = their count)
    int nsrc, npf;
    int spfq[SPLAT_MAX_SOURCES];   // per-frame source inside one 16-byte chunk of the record: that chunk's index, else -1
    int sc0[SPLAT_MAX_SOURCES], scn[SPLAT_MAX_SOURCES], sstride[SPLAT_MAX_SOURCES];
    float *sdf[SPLAT_MAX_SOURCES];
    long long sfs[SPLAT_MAX_SOURCES];
    int depth_channel;
    // CAM > 0 (appended: the CAM = 0 kernels keep their argument offsets): intrinsics and the cameras' frame strides in floats
    const float *intr;
    long long extr_fs, intr_fs;
};

// PF: the row has per-frame sources (A.npf > 0) -- its own instantiation: their block costs the walk ten registers
template <bool ABS, int NCP, bool SETS = false, bool PF = false, int CAM = 0>
__global__ void __launch_bounds__(256, CAM == 0 ? GAUSS_DYN_MINW : GAUSS_DYN_MINW_CAM)
frames_gauss_bwd_dynamic_kernel(const GaussDynArgs A) {
    constexpr int NG = SETS ? SETS_NG : GradLayout<ABS, false>::NG;
    constexpr int NQ = NCP / 4, NS = (NQ + 3) / 4;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t >> 2, j = t & 3;
    if (n >= A.P) return;
    float4 atot[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) atot[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    Cam cam;
    if constexpr (CAM == 0) load_cam(nullptr, A.extr, cam);
    const DynStatic stc = dyn_static(n, j, A.position, A.rotation, A.rot_poly, A.rot_fourier, A.scaling);
    float acc_c[4] = {0.f, 0.f, 0.f, 0.f};  // gradient of the active segment's coefficient rows c0..c3, component j
    float d_pos = 0.f, d_rot = 0.f, d_scl = 0.f, tap_u = 0.f, tap_v = 0.f, atap_u = 0.f, atap_v = 0.f;
    int cur_seg = -1, rmax = 0;
    auto flush = [&](int seg) {
        if (seg < 0 || !A.d_cubic || j >= 3) return;
        const CubicAddr ca = cubic_addr(A.layout, A.P, A.I, seg);
        float *c = A.d_cubic + ca.seg_off + (size_t)n * ca.stride_n + j;
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k * ca.stride_k] += acc_c[k];
    };
    // The frames are walked in groups of (up to) four of one spline segment: the quad sums frame f + k's records and
    // re-evaluates its position / rotation together (lane j = component j), lane k KEEPS frame f + k; then every lane runs
    // the projection / EWA / cov3d / normalisation chain ONCE, for its own frame (the chain on all four lanes for every
    // frame was 4x redundant), and quad sums hand component j of the four frames' results to lane j.
    float scl3[3] = {quad_bcast<0>(stc.scl_j), quad_bcast<1>(stc.scl_j), quad_bcast<2>(stc.scl_j)};
    int f = 0;
    while (f < A.F) {
        const int seg = A.tab[f].seg;
        if (seg != cur_seg) {
            flush(cur_seg);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc_c[k] = 0.f;
            cur_seg = seg;
        }
        if constexpr (CAM > 0) {   // this lane's frame f + j (a lane past the batch reads the last camera; its frame is not valid)
            const size_t fc = (size_t)imin_(f + j, A.F - 1);
            load_cam(CAM == 2 ? A.intr + fc * (size_t)A.intr_fs : nullptr, A.extr + fc * (size_t)A.extr_fs, cam);
        }
        const CubicAddr ca = cubic_addr(A.layout, A.P, A.I, seg);
        float m_ux = 0.f, m_uy = 0.f, m_g3[3] = {0.f, 0.f, 0.f}, m_pos[3] = {0.f, 0.f, 0.f}, m_q[4] = {1.f, 0.f, 0.f, 0.f};
        float m_nrm = 1.f, m_d = 0.f, m_gdep = 0.f;
        bool m_valid = false;
        int took = 0;
        // the slot ranges (and radii) of the group's four frames are requested together: one memory round trip in front of the
        // records' instead of one per frame
        int rb[4], re[4], rr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ff = imin_(f + k, A.F - 1);
            const int *goff = A.goff + (size_t)ff * A.P;
            rb[k] = n > 0 ? goff[n - 1] : 0;
            re[k] = goff[n];
            rr[k] = (A.radii_max && j == 0) ? A.radius[(size_t)ff * A.P + n] : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ff = f + k;
            if (ff >= A.F || A.tab[ff].seg != seg) break;  // grid-uniform
            took = k + 1;
            const int beg = rb[k], end = re[k];
            rmax = imax_(rmax, rr[k]);
            if (end <= beg) continue;  // quad-uniform: no record of this Gaussian in frame ff
            float4 af[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) af[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            const float *base = A.pair + (size_t)ff * (size_t)A.cap * NCP + 4 * j;
            if constexpr (NS == 1) {
                // narrow records: six requested together (one dependent round trip for 94 % of the splats; two at a time was 2 .. 3)
                constexpr int TD = 6;
                for (int r = beg; r < end; r += TD) {
                    float4 v[TD];
#pragma unroll
                    for (int u = 0; u < TD; ++u)
                        v[u] = (r + u < end && j < NQ) ? *reinterpret_cast<const float4 *>(base + (size_t)(r + u) * NCP) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int u = 0; u < TD; ++u) { af[0].x += v[u].x; af[0].y += v[u].y; af[0].z += v[u].z; af[0].w += v[u].w; }
                }
            } else {   // wide records: two in flight (the registers of a third or fourth cost more than the round trips they save)
                int r = beg;
                for (; r + 1 < end; r += 2) {
                    float4 v0[NS], v1[NS];
#pragma unroll
                    for (int c = 0; c < NS; ++c) {
                        const bool mine = 4 * c + j < NQ;
                        v0[c] = mine ? *reinterpret_cast<const float4 *>(base + (size_t)r * NCP + 16 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
                        v1[c] = mine ? *reinterpret_cast<const float4 *>(base + (size_t)(r + 1) * NCP + 16 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
#pragma unroll
                    for (int c = 0; c < NS; ++c) {
                        af[c].x += v0[c].x; af[c].y += v0[c].y; af[c].z += v0[c].z; af[c].w += v0[c].w;
                        af[c].x += v1[c].x; af[c].y += v1[c].y; af[c].z += v1[c].z; af[c].w += v1[c].w;
                    }
                }
                if (r < end) {
#pragma unroll
                    for (int c = 0; c < NS; ++c) {
                        if (4 * c + j < NQ) {
                            const float4 v = *reinterpret_cast<const float4 *>(base + (size_t)r * NCP + 16 * c);
                            af[c].x += v.x; af[c].y += v.y; af[c].z += v.z; af[c].w += v.w;
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                atot[c].x += af[c].x; atot[c].y += af[c].y; atot[c].z += af[c].z; atot[c].w += af[c].w;
            }
            if (SETS && PF) {
                // per-frame sources (track_gs = position(ids2), src/trainer_fragGS.py:506-511): THIS frame's gradient of their
                // channels goes to the frame's own rows; the lane that holds a component adds it (a quad owns its Gaussian)
                for (int g = 0; g < A.nsrc; ++g) {
                    if (A.sfs[g] == 0 || !A.sdf[g]) continue;
                    const int c0 = A.sc0[g], cn = A.scn[g];
                    float *dst = A.sdf[g] + (size_t)ff * (size_t)A.sfs[g] + (size_t)n * A.sstride[g];
                    const int qc = A.spfq[g];
                    if (qc >= 0) {   // at most four channels inside ONE 16-byte chunk of the record (track_gs: chunk 4): one lane adds them
                        float4 v = af[0];
#pragma unroll
                        for (int c = 1; c < NS; ++c)
                            if ((qc >> 2) == c) v = af[c];
                        if (j == (qc & 3)) {
                            const float e4[4] = {v.x, v.y, v.z, v.w};
                            const int e0 = (NG + c0) & 3;
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (e >= e0 && e - e0 < cn) dst[e - e0] += e4[e];
                        }
                        continue;
                    }
#pragma unroll
                    for (int c = 0; c < NS; ++c) {
                        if (4 * c + j < NQ) {
                            const float v[4] = {af[c].x, af[c].y, af[c].z, af[c].w};
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int ch = 16 * c + 4 * j + e - NG;
                                if (ch >= c0 && ch < c0 + cn) dst[ch - c0] += v[e];
                            }
                        }
                    }
                }
            }
            float ux = quad_bcast<0>(af[0].x), uy = quad_bcast<0>(af[0].y);
            float ga = quad_bcast<0>(af[0].z), gb = quad_bcast<0>(af[0].w), gc = quad_bcast<1>(af[0].x);
            float gdep = 0.f;  // SETS: the frame's gradient of the depth channel = dL/ddepth of the projection
            // densification taps: d uv of the whole blend -- SETS records: of the tap set alone (components 8, 9 = chunk 2)
            tap_u += SETS ? quad_bcast<2>(af[0].x) : ux;
            tap_v += SETS ? quad_bcast<2>(af[0].y) : uy;
            if (ABS) {
                atap_u += quad_bcast<1>(af[0].z); atap_v += quad_bcast<1>(af[0].w);
            }
            if (SETS && A.depth_channel >= 0) {
                const int kd = NG + A.depth_channel;  // chunk kd / 4 -> lane (kd / 4) & 3, register af[kd / 16], element kd & 3
                float v = 0.f;
#pragma unroll
                for (int c = 0; c < NS; ++c) {
                    const float e4[4] = {af[c].x, af[c].y, af[c].z, af[c].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (kd == 16 * c + 4 * j + e) v = e4[e];
                }
                gdep = quad_sum(v);
            }
            const float dseg = A.tab[ff].d;
            const DynFrame fr = dyn_frame_rows(n, j, ca, dseg, A.tab[ff].basis, stc, A.cubic);
            if (j == k) {
                m_ux = ux; m_uy = uy; m_g3[0] = ga; m_g3[1] = gb; m_g3[2] = gc;
                m_pos[0] = fr.pos[0]; m_pos[1] = fr.pos[1]; m_pos[2] = fr.pos[2];
                m_q[0] = fr.q[0]; m_q[1] = fr.q[1]; m_q[2] = fr.q[2]; m_q[3] = fr.q[3];
                m_nrm = fr.nrm; m_d = dseg; m_gdep = gdep; m_valid = true;
            }
        }
        f += took;
        // ---- the chain, once per lane for the lane's own frame
        float gp[3] = {0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f}, rq[4] = {0.f, 0.f, 0.f, 0.f};
        if (m_valid) {
            float dq[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (CAM == 2) project_persp_grad_pt(cam, m_pos[0], m_pos[1], m_pos[2], m_ux, m_uy, m_gdep, gp);
            else project_ortho_grad_pt(cam, A.W, A.H, m_ux, m_uy, m_gdep, gp);
            float c3[6], ea[3], eb[3], et[3], Jm[4], cov[3];
            cov3d_pt(scl3, m_q, c3);
            ewa_T<CAM != 2>(cam, m_pos, A.W, A.H, ea, eb, et, Jm);
            ewa_cov2d<CAM != 2>(ea, eb, c3, cov);
            const float det = cov[0] * cov[2] - cov[1] * cov[1];
            if (det != 0.0f) {
                float dcx, dcy, dcz, g6[6];
                ewa_grad_cov_pt(ea, eb, cov, det, m_g3, dcx, dcy, dcz, g6);
                cov3d_grad_pt(scl3, m_q, g6, ds, dq);
                if constexpr (CAM == 2) {   // the conic depends on the frame's position through the Jacobian
                    float ge[3], da[3], db[3], dt[3];
                    ewa_grad_pos_persp_pt(cam, et, ea, eb, c3, dcx, dcy, dcz, ge, da, db, dt);
                    gp[0] += ge[0]; gp[1] += ge[1]; gp[2] += ge[2];
                }
            }
            if (m_nrm < 1e-12f) {
#pragma unroll
                for (int c = 0; c < 4; ++c) rq[c] = dq[c] / 1e-12f;
            } else {
                const float dot = m_q[0] * dq[0] + m_q[1] * dq[1] + m_q[2] * dq[2] + m_q[3] * dq[3];
#pragma unroll
                for (int c = 0; c < 4; ++c) rq[c] = (dq[c] - m_q[c] * dot) / m_nrm;
            }
        }
        // ---- component jj of the four frames' results to lane jj
        const float d1 = m_d, d2 = m_d * m_d, d3 = m_d * m_d * m_d;
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
            const float s0 = quad_sum(gp[jj]), s1 = quad_sum(gp[jj] * d1), s2 = quad_sum(gp[jj] * d2), s3 = quad_sum(gp[jj] * d3);
            const float ss = quad_sum(ds[jj] * scl3[jj]);
            if (j == jj) {
                d_pos += s0;
                acc_c[0] += s3; acc_c[1] += s2; acc_c[2] += s1; acc_c[3] += s0;
                d_scl += ss;
            }
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const float sr = quad_sum(rq[jj]);
            if (j == jj) d_rot += sr;
        }
    }
    flush(cur_seg);
    if (j < 3) {
        if (A.d_position) A.d_position[(size_t)n * 3 + j] += d_pos;
        if (A.d_scaling) A.d_scaling[(size_t)n * 3 + j] += d_scl;
    }
    if (A.d_rotation) A.d_rotation[(size_t)n * 4 + j] += d_rot;
    const float dop = quad_bcast<1>(atot[0].y);
    if (j == 3) {
        if (A.d_opacity) {
            const float s = 1.0f / (1.0f + expf(-A.opacity[n]));
            A.d_opacity[n] += dop * s * (1.0f - s);
        }
        if (A.tap) {
            A.tap[2 * n] = tap_u * (0.5f * (float)A.W);
            A.tap[2 * n + 1] = tap_v * (0.5f * (float)A.H);
        }
        if (ABS && A.abs_tap) {
            A.abs_tap[2 * n] = atap_u * (0.5f * (float)A.W);
            A.abs_tap[2 * n + 1] = atap_v * (0.5f * (float)A.H);
        }
    }
    if (j == 0 && A.radii_max) A.radii_max[n] = rmax;
    if (SETS) {   // shared sources: the sum over the frames (per-frame sources were written frame by frame)
        for (int g = 0; g < A.nsrc; ++g) {
            float *df = A.sdf[g];
            if (!df || A.sfs[g] != 0) continue;
            const int c0 = A.sc0[g], cn = A.scn[g], st = A.sstride[g];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                if (4 * c + j < NQ) {
                    const float v[4] = {atot[c].x, atot[c].y, atot[c].z, atot[c].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ch = 16 * c + 4 * j + e - NG;
                        if (ch >= c0 && ch < c0 + cn && ch != A.depth_channel) df[(size_t)n * st + (ch - c0)] += v[e];
                    }
                }
            }
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        if (4 * c + j < NQ) {
            const int k0 = 16 * c + 4 * j;
            const float v[4] = {atot[c].x, atot[c].y, atot[c].z, atot[c].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ch = k0 + e - NG;
                if (ch >= 0 && ch < A.cn && A.d_feature) {
                    A.d_feature[(size_t)n * A.C + ch] += v[e];
                }
            }
        }
    }
}

// (the library's own events: "gauss_bwd" for the one camera, "gauss_bwd_cam" for CAM > 0)
template <bool ABS, int CAM = 0>
int launch_gauss_bwd_dynamic(const GaussDynArgs &A, int ncp, hipStream_t s) {
    const dim3 grid((unsigned)(((size_t)A.P * 4 + 255) / 256)), block(256);
#define GD(N) case N: SPLAT_LAUNCH(CAM == 0 ? "gauss_bwd" : "gauss_bwd_cam", (frames_gauss_bwd_dynamic_kernel<ABS, N, false, false, CAM>), grid, block, 0, s, A); break
    switch (ncp) {
        GD(8); GD(12); GD(16); GD(20); GD(24); GD(28); GD(32); GD(36); GD(40);
        default: splat_set_error("gauss_bwd: unsupported record stride %d", ncp); return SPLAT_E_ARG;
    }
#undef GD
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

template <int CAM = 0>
int launch_gauss_bwd_dynamic_sets(const GaussDynArgs &A, int ncp, hipStream_t s) {
    const dim3 grid((unsigned)(((size_t)A.P * 4 + 255) / 256)), block(256);
#define GDS(N) case N: if (A.npf > 0) SPLAT_LAUNCH(CAM == 0 ? "gauss_bwd" : "gauss_bwd_cam", (frames_gauss_bwd_dynamic_kernel<true, N, true, true, CAM>), grid, block, 0, s, A); \
                    else SPLAT_LAUNCH(CAM == 0 ? "gauss_bwd" : "gauss_bwd_cam", (frames_gauss_bwd_dynamic_kernel<true, N, true, false, CAM>), grid, block, 0, s, A); break
    switch (ncp) {
        GDS(12); GDS(16); GDS(20); GDS(24); GDS(28); GDS(32); GDS(36); GDS(40);
        default: splat_set_error("gauss_bwd: unsupported record stride %d", ncp); return SPLAT_E_ARG;
    }
#undef GDS
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

}  // namespace
