"""float64 numpy restatements of csrc/flow.hip (include/splat_hip_flow.h): the flow attribute of a batch of frame pairs and its
gradient, the Middlebury colouring (util.flow_to_image), the flow error sums; and the bounds the GPU tests hold the kernels to,
each derived here from the number of float32 roundings of the kernel's chain -- none is fitted to an output.

EPS = 2^-24, the relative error of one float32 rounding."""
import numpy as np

EPS = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------ attribute
# Roundings of one side of a pair, counted in flow.hip: spline position 7 (d d, (d d) d, one fma, two products, two sums, +
# base: 8 operations, the fma rounds once), the camera transform 6 (three products, three sums per row), the pixel map 3
# (orthographic: + 1, * W, - 0.5; the division by 2 is exact) or 5 (pinhole: fx tx, * inv, inv's own rounding, + cx, - 0.5);
# the subtraction uv2 - uv1 rounds once more.  Every rounding is relative to a partial result no larger than the sum of the
# magnitudes of the chain's terms, carried to pixels by the projection's derivative: that sum is A below.  N_ROUND covers the
# longer (pinhole) chain plus the subtraction: 7 + 6 + 5 + 1 = 19, stated as 20.
N_ROUND = 20
DEPTH_MARGIN = 1e-4        # a float64 depth this close to `nearest` may be culled either way in float32 (|z| <= 8: 8 * 13 EPS << 1e-4)
UV_MARGIN = 2e-2           # pixels; a uv this close to an extent threshold likewise (the forward bound below is < 2e-2 px here)


def scalars(clock, times):
    """(segment, d as float64 of the float32 the kernels read) per time"""
    out = [clock.scalars(t) for t in times]
    return np.array([s[0] for s in out]), np.array([np.float32(s[1]) for s in out], np.float64)


def positions(position, cubic, I, seg, d):
    """[F,N,3] float64: position + c3 + c2 d + c1 d^2 + c0 d^3 of the Gaussian-major table [N,4,I,3]; and the sum of the terms'
    magnitudes (what a rounding of the chain is relative to)"""
    c = np.asarray(cubic, np.float64).reshape(-1, 4, I, 3)
    base = np.asarray(position, np.float64)
    F = len(seg)
    p, mag = np.empty((F,) + base.shape), np.empty((F,) + base.shape)
    for f in range(F):
        k = c[:, :, seg[f], :]
        pw = np.array([d[f] ** 3, d[f] ** 2, d[f], 1.0])[None, :, None]
        p[f] = (k * pw).sum(1) + base
        mag[f] = (np.abs(k) * np.abs(pw)).sum(1) + np.abs(base)
    return p, mag


def project(p, mag, extr, intr, W, H, nearest, extent):
    """the project's projection rules in float64 (tests/torch_twin.py: project_point_ortho / project_point_persp) for points
    [N,3] under one camera: uv [N,2] before the cull, cull [N], near [N] (a decision within the margins), J [N,2,3] = duv/dp,
    A [N,2] = the pixel-scale magnitude of the chain (see N_ROUND)"""
    e = np.asarray(extr, np.float64).reshape(-1)[:12].reshape(3, 4)
    R, t = e[:, :3], e[:, 3]
    cam = p @ R.T + t
    cam_mag = mag @ np.abs(R).T + np.abs(t)
    N = p.shape[0]
    J = np.empty((N, 2, 3))
    if intr is None:
        sx, sy = W / 2.0, H / 2.0
        u, v = (cam[:, 0] + 1.0) * sx - 0.5, (cam[:, 1] + 1.0) * sy - 0.5
        J[:, 0], J[:, 1] = sx * R[0], sy * R[1]
        A = np.stack([sx * (cam_mag[:, 0] + 1.0) + 0.5, sy * (cam_mag[:, 1] + 1.0) + 0.5], 1)
        cull = cam[:, 2] <= nearest
        near = np.abs(cam[:, 2] - nearest) < DEPTH_MARGIN
        ext = True
    else:
        fx, fy, cx, cy = (float(x) for x in np.asarray(intr, np.float64).reshape(-1)[:4])
        z = cam[:, 2] + 1e-7
        u, v = fx * cam[:, 0] / z + cx - 0.5, fy * cam[:, 1] / z + cy - 0.5
        J[:, 0] = (fx / z)[:, None] * R[0] - (fx * cam[:, 0] / z ** 2)[:, None] * R[2]
        J[:, 1] = (fy / z)[:, None] * R[1] - (fy * cam[:, 1] / z ** 2)[:, None] * R[2]
        A = np.stack([np.abs(fx / z) * cam_mag[:, 0] + np.abs(fx * cam[:, 0] / z ** 2) * cam_mag[:, 2] + abs(cx) + 0.5,
                      np.abs(fy / z) * cam_mag[:, 1] + np.abs(fy * cam[:, 1] / z ** 2) * cam_mag[:, 2] + abs(cy) + 0.5], 1)
        cull = (cam[:, 2] <= nearest) if nearest > 0 else np.zeros(N, bool)
        near = (np.abs(cam[:, 2] - nearest) < DEPTH_MARGIN) if nearest > 0 else np.zeros(N, bool)
        ext = extent > 0
    if ext:
        for x, S in ((u, W), (v, H)):
            lo, hi = (1 - extent) * S * 0.5, (1 + extent) * S * 0.5
            cull = cull | (x < lo) | (x > hi)
            near = near | (np.abs(x - lo) < UV_MARGIN) | (np.abs(x - hi) < UV_MARGIN)
    return np.stack([u, v], 1), cull, near, J, A


def _pick(c, f, per_frame_ndim):
    return None if c is None else (c[f] if np.ndim(c) == per_frame_ndim else c)


def attribute(clock, times1, times2, position, cubic, extr, intr, extr2, intr2, W, H, nearest=0.01, extent=1.3,
              zero_culled=False, g=None):
    """float64 flow attribute [F,N,2] of F pairs (cubic Gaussian-major [N, 4 I 3]); extr [4,4] or [F,4,4], intr None / [4] /
    [F,4]; extr2 / intr2 None: the first camera's.  Returns a dict: flow, uv1, uv2 (zeroed where culled), cull1, cull2, near
    (a cull decision of either side within the margins), bound (per element: N_ROUND EPS (A1 + A2), a culled side left out); with ``g`` [F,N,2] also
    d_position [N,3] and d_cubic [N,4,I,3] (a culled side contributes zero)."""
    I = clock.interval_num
    F, N = len(times1), np.shape(position)[0]
    e2 = extr if extr2 is None else extr2
    i2 = intr if intr2 is None else intr2
    out = dict(flow=np.zeros((F, N, 2)), uv1=np.zeros((F, N, 2)), uv2=np.zeros((F, N, 2)), cull1=np.zeros((F, N), bool),
               cull2=np.zeros((F, N), bool), near=np.zeros((F, N), bool), bound=np.zeros((F, N, 2)))
    if g is not None:
        out["d_position"], out["d_cubic"] = np.zeros((N, 3)), np.zeros((N, 4, I, 3))
    sides = []
    for times in (times1, times2):
        seg, d = scalars(clock, times)
        sides.append((seg, d) + positions(position, cubic, I, seg, d))
    for f in range(F):
        pr = []
        for s, (e, i_) in enumerate(((extr, intr), (e2, i2))):
            seg, d, p, mag = sides[s]
            pr.append(project(p[f], mag[f], _pick(e, f, 3), _pick(i_, f, 2), W, H, nearest, extent))
        (uv1, c1, n1, J1, A1), (uv2, c2, n2, J2, A2) = pr
        uv1, uv2 = uv1 * ~c1[:, None], uv2 * ~c2[:, None]
        flow = uv2 - uv1
        dead = (c1 | c2) if zero_culled else np.zeros(N, bool)
        flow[dead] = 0.0
        out["flow"][f], out["uv1"][f], out["uv2"][f] = flow, uv1, uv2
        out["cull1"][f], out["cull2"][f], out["near"][f] = c1, c2, n1 | n2
        out["bound"][f] = N_ROUND * EPS * (A1 * ~(c1 | dead)[:, None] + A2 * ~(c2 | dead)[:, None])      # a culled side is an exact 0
        if g is not None:
            for s, (J, cull, sign) in enumerate(((J1, c1, -1.0), (J2, c2, 1.0))):
                seg, d = sides[s][0][f], sides[s][1][f]
                gp = sign * np.einsum("nc,ncj->nj", np.asarray(g[f], np.float64), J) * (~(cull | dead))[:, None]
                out["d_position"] += gp
                for k in range(4):
                    out["d_cubic"][:, k, seg, :] += gp * d ** (3 - k)
    return out


def gamma(ref):
    """the forward bound in the issue's form |err| <= gamma (|uv1| + |uv2| + 1): gamma = N_ROUND EPS kappa, kappa the largest
    ratio of the chain's pixel-scale magnitude to |uv1| + |uv2| + 1 over the scene (float64 quantities of the inputs only)"""
    den = np.abs(ref["uv1"]) + np.abs(ref["uv2"]) + 1.0
    return float((ref["bound"] / den).max())


# ------------------------------------------------------------------------------------------------------------ colours
def colorwheel():
    """Scharstein's wheel: 55 rows (r, g, b) in 0 .. 255, six ramps of 15, 6, 4, 11, 13, 6 steps"""
    rows = []
    for n, fixed, ramp, down in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False),
                                 (6, 0, 2, True)):
        for k in range(n):
            r = [0.0, 0.0, 0.0]
            r[fixed] = 255.0
            step = np.floor(255.0 * k / n)
            r[ramp] = 255.0 - step if down else step
            rows.append(r)
    return np.array(rows, np.float64)


WHEEL = colorwheel()
# Margin of the byte comparison, in levels of the pre-floor value 255 col.  Angle: u / den and v / den round once each (2 EPS
# of an angle <= pi), atan2f is taken as accurate to ATAN_ULPS units of 2^-22 (the spacing of float32 next to pi), a = angle /
# pi, a + 1, / 2 * 54 round once each on values <= 54 (half-spacing 2^-19).  The wheel's steepest ramp is the 4-step green-cyan
# one: 64 levels per unit of fk.  Radius: u^2, v^2, their sum, the square root on top of the two divisions: 6 EPS relative, on
# a term <= 255 levels.
ATAN_ULPS = 4
FK_ERR = 27.0 / np.pi * (ATAN_ULPS * 2.0 ** -22 + 2 * EPS * np.pi) + 3 * 2.0 ** -19
STEEPEST = float(np.abs(np.diff(np.vstack([WHEEL, WHEEL[:1]]), axis=0)).max())
RAD_ERR = 255.0 * 6 * EPS
LEVEL_MARGIN = STEEPEST * FK_ERR + RAD_ERR      # the widest margin; a channel on a flatter ramp has its own (colours())


def colours(flow, clip_flow=None, scale="per_frame", bgr=False):
    """float64 restatement of util.flow_to_image on maps [T,2,H,W]: returns (bytes [T,H,W,3], pre = 255 col before the floor
    [T,H,W,3], exact [T,H,W,3]: the channel is exactly 255 (or, beyond the wheel, exactly 0) whatever the roundings (zero radius, or both wheel entries 255 --
    and the entry before them where fk is within FK_ERR of a bin border), margin [T,H,W,3]: the channel's own margin in levels -- the slope of ITS ramp segment (the
    steepest one where fk is within FK_ERR of a bin border) times FK_ERR, plus RAD_ERR --, rad_max [T]).  A non-finite pixel:
    black, left out of the maximum."""
    f = np.asarray(flow, np.float64)
    if clip_flow is not None:
        f = np.clip(f, 0.0, float(clip_flow))
    u, v = f[:, 0], f[:, 1]
    ok = np.isfinite(u) & np.isfinite(v)
    rad = np.where(ok, np.sqrt(np.where(ok, u, 0) ** 2 + np.where(ok, v, 0) ** 2), 0.0)
    T = f.shape[0]
    if scale == "per_frame":
        rmax = rad.reshape(T, -1).max(1)
    elif scale == "whole_clip":
        rmax = np.full(T, rad.max())
    else:
        rmax = np.full(T, float(np.float32(scale)))
    den = (rmax + np.float64(np.float32(1e-5)))[:, None, None]
    u, v = np.where(ok, u, 0) / den, np.where(ok, v, 0) / den
    rad = np.sqrt(u * u + v * v)
    fk = (np.arctan2(-v, -u) / np.pi + 1.0) / 2.0 * 54.0
    k0 = np.clip(np.floor(fk).astype(np.int64), 0, 54)
    k1 = np.where(k0 == 54, 0, k0 + 1)
    fr = (fk - k0)[..., None]
    c0, c1 = WHEEL[k0] / 255.0, WHEEL[k1] / 255.0
    col = (1.0 - fr) * c0 + fr * c1
    inside = (rad <= 1.0)[..., None]
    col = np.where(inside, 1.0 - rad[..., None] * (1.0 - col), col * 0.75)
    pre = 255.0 * col * ok[..., None]
    clear = (np.abs(fk - np.round(fk)) > FK_ERR)[..., None]
    margin = np.where(clear, np.abs(WHEEL[k1] - WHEEL[k0]), STEEPEST) * FK_ERR + RAD_ERR
    sat = (WHEEL[k0] == 255.0) & (WHEEL[k1] == 255.0)           # next to a bin border: the bin before k0 as well
    exact = ok[..., None] & inside & ((rad == 0.0)[..., None] | (sat & (clear | (WHEEL[(k0 - 1) % 55] == 255.0))))
    # beyond the wheel (col * 0.75) a channel whose wheel entries are both 0 is an exact 0
    none = (WHEEL[k0] == 0.0) & (WHEEL[k1] == 0.0) & (clear | (WHEEL[(k0 - 1) % 55] == 0.0))
    exact = exact | (ok[..., None] & ~inside & (np.abs(rad - 1.0) > 8 * EPS)[..., None] & none)
    img = np.floor(pre).astype(np.uint8)
    if bgr:
        img, pre, exact, margin = img[..., ::-1], pre[..., ::-1], exact[..., ::-1], margin[..., ::-1]
    return img, pre, exact, margin, rmax


def decided(pre, exact, margin):
    """bytes the comparison holds to equality: the float64 pre-floor value is farther than the channel's margin from an integer,
    or the channel is an exact 255"""
    return (np.abs(pre - np.round(pre)) > margin) | exact


# ------------------------------------------------------------------------------------------------------------ error
PARTIAL_N = 2048          # pixels a workgroup sums in float32 (256 threads x 8 pixels)
# Roundings on the way of a term into a partial: per term at most 5 (du, dv, their squares' sum / |du| + |dv|, the square root,
# * w), per thread 8 sequential additions, 6 levels of the wave tree, 3 additions of the four wave totals = 22; all terms are
# >= 0, so the error is relative to the sum itself.  The float64 fold of the partials adds nothing visible at this scale.
SUM_ROUNDINGS = 24


def error_sums(pred, gt, weight=None, scale=1.0):
    """(sums [T,3] float64: sum w (|du| + |dv|), sum w sqrt(du^2 + dv^2), sum w; grad [T,2,H,W] = scale w sign(d) / max(sum w,
    1e-30)) of maps [T,2,H,W]"""
    d = np.asarray(pred, np.float64) - np.asarray(gt, np.float64)
    T = d.shape[0]
    w = np.ones((T,) + d.shape[2:]) if weight is None else np.asarray(weight, np.float64).reshape((T,) + d.shape[2:])
    sums = np.stack([(w * (np.abs(d[:, 0]) + np.abs(d[:, 1]))).reshape(T, -1).sum(1),
                     (w * np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)).reshape(T, -1).sum(1), w.reshape(T, -1).sum(1)], 1)
    grad = scale * w[:, None] * np.sign(d) / np.maximum(sums[:, 2], 1e-30)[:, None, None, None]
    return sums, grad
