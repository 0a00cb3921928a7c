"""numpy restatements of the entry points of include/splat_hip_flow_occ.h (csrc/flow.hip): the flow attribute with the depth and
its gradient in float64, built on tests/flow_ref.py, with the bound of the depth channels derived from the kernel's chain; and
the fused occlusion kernel twice -- in float32, operation for operation (the kernel is compiled without contraction, so its
floats are THESE bits and its decisions follow), and in float64 (the twin the float32 one is held against)."""
import numpy as np

import flow_ref as FR

EPS = FR.EPS
OUTSIDE, UNCOVERED, IN_FRONT, INCONSISTENT = 1, 2, 4, 8

# ------------------------------------------------------------------------------------------------------------ attribute
# Roundings of the depth of one side, counted in flow.hip as flow_ref counts the uv chain: spline position 7, the camera
# transform's z row 6 (three products, three sums); the depth is the transformed z itself, for both camera kinds.  z2 - z1
# rounds once more: 7 + 6 + 1 = 14, stated as 15.  Every rounding is relative to a partial result no larger than the sum of the
# magnitudes of the chain's terms: A_z below.
N_ROUND_Z = 15


def depth_row(p, mag, extr):
    """float64 camera-space z [N] of points [N,3] under one camera, its magnitude sum A_z [N] and dz/dp [3]"""
    e = np.asarray(extr, np.float64).reshape(-1)[:12].reshape(3, 4)
    return p @ e[2, :3] + e[2, 3], mag @ np.abs(e[2, :3]) + abs(e[2, 3]), e[2, :3]


def attribute4(clock, times1, times2, position, cubic, extr, intr, extr2, intr2, W, H, nearest=0.01, extent=1.3, zero_culled=False,
               g=None):
    """float64 [F,N,4] = (u2 - u1, v2 - v1, z2 - z1, z2): flow_ref.attribute's dict (channels 0, 1, the cull decisions, `near`)
    with ``attr`` [F,N,4], ``z1`` / ``z2`` (zeroed where culled) and ``bound`` [F,N,4] (channels 2, 3: N_ROUND_Z EPS times the
    A_z of the sides that are not an exact 0); with ``g`` [F,N,4] also d_position and d_cubic of the whole row (the depth of side
    1 receives -g[2], of side 2 g[2] + g[3]; a culled side contributes zero)."""
    I = clock.interval_num
    F, N = len(times1), np.shape(position)[0]
    g = None if g is None else np.asarray(g, np.float64)
    out = FR.attribute(clock, times1, times2, position, cubic, extr, intr, extr2, intr2, W, H, nearest, extent, zero_culled,
                       g=None if g is None else g[..., :2])
    e2 = extr if extr2 is None else extr2
    out["z1"], out["z2"] = np.zeros((F, N)), np.zeros((F, N))
    attr, bound = np.zeros((F, N, 4)), np.zeros((F, N, 4))
    attr[..., :2], bound[..., :2] = out["flow"], out["bound"]
    sides = []
    for times in (times1, times2):
        seg, d = FR.scalars(clock, times)
        sides.append((seg, d) + FR.positions(position, cubic, I, seg, d))
    for f in range(F):
        c1, c2 = out["cull1"][f], out["cull2"][f]
        dead = (c1 | c2) if zero_culled else np.zeros(N, bool)
        zs = []
        for s, (e, cull) in enumerate(((extr, c1), (e2, c2))):
            seg, d, p, mag = sides[s]
            z, Az, dz = depth_row(p[f], mag[f], FR._pick(e, f, 3))
            live = ~(cull | dead)
            zs.append((z * ~cull, Az * live))
            if g is not None:
                gz = -g[f, :, 2] if s == 0 else g[f, :, 2] + g[f, :, 3]
                gp = (gz * live)[:, None] * dz[None, :]
                out["d_position"] += gp
                for k in range(4):
                    out["d_cubic"][:, k, seg[f], :] += gp * d[f] ** (3 - k)
        (z1, A1), (z2, A2) = zs
        out["z1"][f], out["z2"][f] = z1, z2
        attr[f, :, 2], attr[f, :, 3] = (z2 - z1) * ~dead, z2 * ~dead
        bound[f, :, 2], bound[f, :, 3] = N_ROUND_Z * EPS * (A1 + A2), N_ROUND_Z * EPS * A2
    out["attr"], out["bound"] = attr, bound
    return out


# ------------------------------------------------------------------------------------------------------------ fused kernel
def bilinear(plane, qx, qy, dt):
    """B(plane, q) of planes [..., H, W] at in-range q (arrays of the leading shape's pixels), every operation in ``dt``:
    x0 = floor(qx), x1 = min(x0 + 1, W - 1), fx = qx - x0, likewise y;
    B = ((v00 (1 - fx)) + (v01 fx)) (1 - fy) + ((v10 (1 - fx)) + (v11 fx)) fy.  Returns (B, |v00| + |v01| + |v10| + |v11|)."""
    plane = np.asarray(plane, dt)
    H, W = plane.shape[-2:]
    qx, qy = np.asarray(qx, dt), np.asarray(qy, dt)
    x0f, y0f = np.floor(qx), np.floor(qy)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = qx - x0f, qy - y0f
    gx, gy = dt(1) - fx, dt(1) - fy
    v00, v01, v10, v11 = plane[..., y0, x0], plane[..., y0, x1], plane[..., y1, x0], plane[..., y1, x1]
    B = ((v00 * gx) + (v01 * fx)) * gy + ((v10 * gx) + (v11 * fx)) * fy
    return B, np.abs(v00) + np.abs(v01) + np.abs(v10) + np.abs(v11)


def occlusion(flow, track_depth=None, surface=None, coverage=None, flow_back=None, src=None, bg_depth=1.0, depth_margin=0.05,
              min_coverage=0.5, fb_alpha=0.01, fb_beta=0.5, dt=np.float32):
    """splat_flow_occlusion on maps [F,2,H,W] with every operation in ``dt`` (np.float32: the kernel's bits; np.float64: the
    twin).  Returns a dict: mask uint8 [F,H,W], depth_gap, fb_sq [F,H,W], warped [F,C,H,W] (None without their inputs), counts
    int [F,4]."""
    flow = np.asarray(flow, dt)
    F, _, H, W = flow.shape
    bg_depth, depth_margin, min_coverage, fb_alpha, fb_beta = (dt(x) for x in (bg_depth, depth_margin, min_coverage, fb_alpha, fb_beta))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = dict(mask=np.zeros((F, H, W), np.uint8), depth_gap=None, fb_sq=None, warped=None, counts=np.zeros((F, 4), np.int64))
    if surface is not None:
        out["depth_gap"] = np.zeros((F, H, W), dt)
    if flow_back is not None:
        out["fb_sq"] = np.zeros((F, H, W), dt)
    if src is not None:
        out["warped"] = np.zeros((F,) + np.shape(src)[1:], dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(F):
            u, v = flow[f, 0], flow[f, 1]
            qx, qy = xs.astype(dt) + u, ys.astype(dt) + v
            inside = (qx >= 0) & (qx <= dt(W - 1)) & (qy >= 0) & (qy <= dt(H - 1))
            bits = np.where(inside, 0, OUTSIDE).astype(np.uint8)
            cov = None
            if coverage is not None:
                cov = np.asarray(coverage, dt).reshape(F, H, W)[f]
                bits |= np.where(cov >= min_coverage, 0, UNCOVERED).astype(np.uint8)
            decide = bits == 0
            sx, sy = np.where(inside, qx, dt(0)), np.where(inside, qy, dt(0))     # nothing is sampled outside
            if surface is not None:
                s, _ = bilinear(np.asarray(surface, dt).reshape(F, H, W)[f], sx, sy, dt)
                td = np.asarray(track_depth, dt).reshape(F, H, W)[f]
                if cov is not None:
                    td = td + (dt(1) - cov) * bg_depth
                gap = np.where(inside, td - s, dt(0))
                out["depth_gap"][f] = gap
                bits |= np.where(decide & (gap > depth_margin), IN_FRONT, 0).astype(np.uint8)
            if flow_back is not None:
                fbk = np.asarray(flow_back, dt)[f]
                bu, _ = bilinear(fbk[0], sx, sy, dt)
                bv, _ = bilinear(fbk[1], sx, sy, dt)
                uu, vv = np.where(inside, u, dt(0)), np.where(inside, v, dt(0))
                ru, rv = uu + bu, vv + bv
                fb = ru * ru + rv * rv
                lim = fb_alpha * ((uu * uu + vv * vv) + (bu * bu + bv * bv)) + fb_beta
                out["fb_sq"][f] = np.where(inside, fb, dt(0))
                bits |= np.where(decide & (fb > lim), INCONSISTENT, 0).astype(np.uint8)
            if src is not None:
                w, _ = bilinear(np.asarray(src, dt)[f], sx, sy, dt)
                out["warped"][f] = np.where(inside[None], w, dt(0))
            out["mask"][f] = bits
            out["counts"][f] = [int(((bits >> t) & 1).sum()) for t in range(4)]
    return out
