"""Independent float64 PyTorch twin of the rasterizer ops (test helper).

Written from the operator SEMANTICS, vectorised over the pixels of a tile,
so that torch.autograd provides gradients to cross-check the analytic backward passes of the C
oracle (oracle/splat_oracle.c) and of the HIP kernels.  Not a product path.
"""
from __future__ import annotations

import torch

TILE = 16


def project_point_persp(xyz, intr, extr, W, H, nearest=0.2, extent=1.3):
    R = extr[:3, :3]
    t = xyz @ R.T + extr[:3, 3]
    inv = 1.0 / (t[:, 2] + 1e-7)
    u = intr[0] * t[:, 0] * inv + intr[2] - 0.5
    v = intr[1] * t[:, 1] * inv + intr[3] - 0.5
    d = t[:, 2]
    cull = torch.zeros_like(d, dtype=torch.bool)
    if nearest > 0:
        cull |= d <= nearest
    if extent > 0:
        cull |= (u < (1 - extent) * W * 0.5) | (u > (1 + extent) * W * 0.5)
        cull |= (v < (1 - extent) * H * 0.5) | (v > (1 + extent) * H * 0.5)
    keep = (~cull).to(xyz.dtype)
    uv = torch.stack([u, v], -1) * keep[:, None]
    return uv, (d * keep)[:, None]


def project_point_ortho(xyz, extr, W, H, nearest=0.01, extent=1.3):
    R = extr[:3, :3]
    t = xyz @ R.T + extr[:3, 3]
    u = (t[:, 0] + 1.0) * W / 2 - 0.5
    v = (t[:, 1] + 1.0) * H / 2 - 0.5
    d = t[:, 2]
    cull = (d <= nearest)
    cull |= (u < (1 - extent) * W * 0.5) | (u > (1 + extent) * W * 0.5)
    cull |= (v < (1 - extent) * H * 0.5) | (v > (1 + extent) * H * 0.5)
    keep = (~cull).to(xyz.dtype)
    return torch.stack([u, v], -1) * keep[:, None], (d * keep)[:, None]


def quat_to_R(q):
    r, x, y, z = q.unbind(-1)
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def cov3d(scale, quat, visible=None):
    R = quat_to_R(quat)
    L = R * scale[:, None, :]
    S = L @ L.transpose(1, 2)
    out = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)
    if visible is not None:
        out = out * visible.reshape(-1, 1).to(out.dtype)
    return out


def _sym(c):
    return torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]],
                       -1).reshape(-1, 3, 3)


def ewa(xyz, cov3, intr, extr, W, H, mask, ortho=False):
    """conic only (radius / tiles are not differentiable); mask = radius>0 from the oracle."""
    R = extr[:3, :3]
    t = xyz @ R.T + extr[:3, 3]
    P = xyz.shape[0]
    J = torch.zeros(P, 2, 3, dtype=xyz.dtype)
    if ortho:
        J[:, 0, 0] = W / 2
        J[:, 1, 1] = H / 2
    else:
        J[:, 0, 0] = intr[0] / t[:, 2]
        J[:, 1, 1] = intr[1] / t[:, 2]
        J[:, 0, 2] = -intr[0] * t[:, 0] / t[:, 2] ** 2
        J[:, 1, 2] = -intr[1] * t[:, 1] / t[:, 2] ** 2
    T = J @ R
    c = T @ _sym(cov3) @ T.transpose(1, 2)
    a = c[:, 0, 0] + 0.3
    b = c[:, 0, 1]
    d = c[:, 1, 1] + 0.3
    det = a * d - b * b
    conic = torch.stack([d / det, -b / det, a / det], -1)
    return conic * mask.reshape(-1, 1).to(conic.dtype)


def sh_color(shs, deg, dirs, free=False):
    C0 = 0.28209479177387814
    C1 = 0.4886025119029199
    C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
    C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
          1.445305721320277, -0.5900435899266435]
    x, y, z = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    r = C0 * shs[:, 0]
    if deg > 0:
        r = r - C1 * y * shs[:, 1] + C1 * z * shs[:, 2] - C1 * x * shs[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = r + C2[0] * xy * shs[:, 4] + C2[1] * yz * shs[:, 5] + C2[2] * (2 * zz - xx - yy) * shs[:, 6] + \
            C2[3] * xz * shs[:, 7] + C2[4] * (xx - yy) * shs[:, 8]
    if deg > 2:
        r = r + C3[0] * y * (3 * xx - yy) * shs[:, 9] + C3[1] * xy * z * shs[:, 10] + \
            C3[2] * y * (4 * zz - xx - yy) * shs[:, 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * shs[:, 12] + \
            C3[4] * x * (4 * zz - xx - yy) * shs[:, 13] + C3[5] * z * (xx - yy) * shs[:, 14] + \
            C3[6] * x * (xx - 3 * yy) * shs[:, 15]
    if free:
        return r
    return torch.clamp_min(r + 0.5, 0.0)


def blend(uv, conic, opacity, feature, idx_sorted, tile_range, bg, W, H, bias=None, K=0, truncate=False):
    """Front-to-back compositing (Appendix A.6). Returns out[C,H,W], final_T[H,W], ncontrib[H,W], gs_idx.
    The 0.99 clamp is straight-through (the reference does not mask it in the gradient)."""
    dt = uv.dtype
    C = feature.shape[1]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    out = torch.zeros(C, H, W, dtype=dt)
    fT = torch.zeros(H, W, dtype=dt)
    nc = torch.zeros(H, W, dtype=torch.int32)
    gi = torch.full((H, W, max(K, 1)), -1, dtype=torch.int32)
    opacity = opacity.reshape(-1)
    for tile in range(gx * gy):
        tx, ty = tile % gx, tile // gx
        x0, y0 = tx * TILE, ty * TILE
        x1, y1 = min(W, x0 + TILE), min(H, y0 + TILE)
        ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        px = xs.reshape(-1).to(dt)
        py = ys.reshape(-1).to(dt)
        n = px.numel()
        T = torch.ones(n, dtype=dt)
        F = torch.zeros(n, C, dtype=dt)
        done = torch.zeros(n, dtype=torch.bool)
        last = torch.zeros(n, dtype=torch.int32)
        layer = torch.zeros(n, dtype=torch.long)
        gsl = torch.full((n, max(K, 1)), -1, dtype=torch.int32)
        r0, r1 = int(tile_range[tile, 0]), int(tile_range[tile, 1])
        contributor = 0
        for s in range(r0, r1):
            contributor += 1
            if bool(done.all()):
                break
            g = int(idx_sorted[s])
            dx = uv[g, 0] - px
            dy = uv[g, 1] - py
            power = -0.5 * (conic[g, 0] * dx * dx + conic[g, 2] * dy * dy) - conic[g, 1] * dx * dy
            araw = opacity[g] * torch.exp(power)
            if bias is not None:
                araw = araw + bias.reshape(-1)[g]
            alpha = araw + (torch.clamp_max(araw, 0.99) - araw).detach()
            ok = (~done) & (power <= 0) & (alpha >= 1.0 / 255.0)
            nT = T * (1 - alpha)
            sat = ok & (nT < 1e-4)
            done = done | sat
            app = ok & ~sat
            w = torch.where(app, alpha * T, torch.zeros_like(T))
            F = F + w[:, None] * feature[g][None, :]
            T = torch.where(app, nT, T)
            last = torch.where(app, torch.full_like(last, contributor), last)
            if K > 0:
                rec = app & (layer < K)
                if bool(rec.any()):
                    ridx = torch.nonzero(rec).reshape(-1)
                    gsl[ridx, layer[ridx]] = g
                    layer = layer + rec.long()
                if truncate:
                    done = done | (app & (layer >= K))
        out[:, y0:y1, x0:x1] = (F + T[:, None] * bg).T.reshape(C, y1 - y0, x1 - x0)
        fT[y0:y1, x0:x1] = T.detach().reshape(y1 - y0, x1 - x0)
        nc[y0:y1, x0:x1] = last.reshape(y1 - y0, x1 - x0)
        gi[y0:y1, x0:x1] = gsl.reshape(y1 - y0, x1 - x0, -1)
    return out, fT, nc, gi


# ------------------------------------------------------------------ per-Gaussian geometry with its decisions (float64)
# Everything below restates the operators' semantics once more with what a strict comparison needs besides the values:
# the integer outputs, the float64 distance of every row to each discrete decision, and absolute-value companions
# (every product and sum taken over magnitudes) that bound what float32 rounding can do to a row.
F32_MAX = 3.4028234663852886e38


def _f32(x):
    import numpy as np
    return np.float32(x)


def cull_bounds(W, H, extent, ortho):
    """the four extent bounds exactly as the float32 operators form them (constants, not per-row arithmetic): the
    pinhole operator multiplies (1 -+ extent) * W in float32 and halves in double, the orthographic one works in double"""
    e = _f32(extent)
    if ortho:
        lo = lambda n: float(_f32((1.0 - float(e)) * n * 0.5))
        hi = lambda n: float(_f32((1.0 + float(e)) * n * 0.5))
    else:
        lo = lambda n: float(_f32(float((_f32(1) - e) * _f32(n)) * 0.5))
        hi = lambda n: float(_f32(float((_f32(1) + e) * _f32(n)) * 0.5))
    return lo(W), hi(W), lo(H), hi(H)


def cam_xform(xyz, extr):
    return xyz @ extr[:3, :3].T + extr[:3, 3]


def cam_xform_abs(xyz, extr):
    return xyz.abs() @ extr[:3, :3].abs().T + extr[:3, 3].abs()


def project_full(xyz, intr, extr, W, H, nearest, extent, ortho):
    """uv, depth (zero where culled), the cull flag, and per decision its signed float64 distance ``dist`` together with
    the magnitude ``mag`` that float32 rounding of the compared quantity scales with"""
    t = cam_xform(xyz, extr)
    ta = cam_xform_abs(xyz, extr)
    tz = t[:, 2]
    if ortho:
        u = (t[:, 0] + 1.0) * W / 2 - 0.5
        v = (t[:, 1] + 1.0) * H / 2 - 0.5
        d = torch.nan_to_num(tz, nan=0.0, posinf=F32_MAX, neginf=-F32_MAX)
        mu = (ta[:, 0] + 1.0) * W / 2 + 0.5
        mv = (ta[:, 1] + 1.0) * H / 2 + 0.5
    else:
        inv = 1.0 / (tz + 1e-7)
        u = intr[0] * t[:, 0] * inv + intr[2] - 0.5
        v = intr[1] * t[:, 1] * inv + intr[3] - 0.5
        d = tz
        ai = inv.abs()
        mu = intr[0].abs() * ai * (ta[:, 0] + t[:, 0].abs() * ta[:, 2] * ai) + intr[2].abs() + 0.5
        mv = intr[1].abs() * ai * (ta[:, 1] + t[:, 1].abs() * ta[:, 2] * ai) + intr[3].abs() + 0.5
    xlo, xhi, ylo, yhi = cull_bounds(W, H, extent, ortho)
    near = float(_f32(nearest))
    cull = torch.zeros_like(d, dtype=torch.bool)
    dist, mag = {}, {}
    if ortho or nearest > 0:
        cull |= d <= near
        dist["near"], mag["near"] = d - near, ta[:, 2]
    if ortho or extent > 0:
        cull |= (u < xlo) | (u > xhi) | (v < ylo) | (v > yhi)
        dist.update(ulo=u - xlo, uhi=xhi - u, vlo=v - ylo, vhi=yhi - v)
        mag.update(ulo=mu, uhi=mu, vlo=mv, vhi=mv)
    keep = ~cull
    z = torch.zeros_like(u)
    uv = torch.stack([torch.where(keep, u, z), torch.where(keep, v, z)], -1)
    depth = torch.where(keep, d, z)[:, None]
    return dict(uv=uv, depth=depth, cull=cull, dist=dist, mag=mag, u=u, v=v, mag_u=mu, mag_v=mv)


def quat_to_R_abs(q):
    r, x, y, z = q.abs().unbind(-1)
    return torch.stack([
        1 + 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 + 2 * (x * x + z * z), 2 * (y * z + r * x),
        2 * (x * z + r * y), 2 * (y * z + r * x), 1 + 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def cov3d_abs(scale, quat):
    """|R| S^2 |R|^T with the entries of R taken over magnitudes: the float32 error of a cov3d element is a few ulp of this"""
    L = quat_to_R_abs(quat) * scale.abs()[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)


def _ewa_T(xyz, intr, extr, W, H, ortho, vis=None):
    R = extr[:3, :3]
    t = cam_xform(xyz, extr)
    if vis is not None:      # invisible rows (behind the camera, non-finite) take no part: keep their arithmetic finite
        t = torch.where(vis[:, None], t, torch.tensor([0.0, 0.0, 1.0], dtype=t.dtype).expand_as(t))
    P = xyz.shape[0]
    J = torch.zeros(P, 2, 3, dtype=xyz.dtype)
    if ortho:
        J[:, 0, 0] = W / 2
        J[:, 1, 1] = H / 2
    else:
        J[:, 0, 0] = intr[0] / t[:, 2]
        J[:, 1, 1] = intr[1] / t[:, 2]
        J[:, 0, 2] = -intr[0] * t[:, 0] / t[:, 2] ** 2
        J[:, 1, 2] = -intr[1] * t[:, 1] / t[:, 2] ** 2
    return J @ R, J.abs() @ R.abs()


def tile_rect(px, py, r, W, H):
    """tile rectangle of a splat: division by the tile size truncated toward zero, then clamped to the grid; besides the
    rectangle the four quotients before truncation (the decisions)"""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    q = torch.stack([(px - r) / TILE, (py - r) / TILE, (px + r + TILE - 1.0) / TILE, (py + r + TILE - 1.0) / TILE], -1)
    g = torch.tensor([gx, gy, gx, gy], dtype=torch.int64)
    rect = torch.minimum(torch.clamp_min(torch.trunc(torch.nan_to_num(q, nan=0.0, posinf=1e9, neginf=-1e9)).to(torch.int64), 0), g)
    return rect, q, g


def ewa_full(xyz, cov3, intr, extr, uv, W, H, visible, ortho, cov3_mag=None):
    """every output of the EWA projection and what decides it.  ``conic`` is differentiable (zero on dead rows);
    ``live`` = visible, det != 0 and a non-empty tile rectangle.  ``kappa`` is the row's conditioning: the first-order change of the 2-D determinant
    when each element of T Sigma T^T moves by its sum of magnitudes |T| |Sigma| |T|^T (``cov3_mag`` in place of |Sigma|
    when the 3-D covariance is itself computed in float32), relative to the determinant."""
    vis = visible.reshape(-1).bool()
    T, Ta = _ewa_T(xyz, intr, extr, W, H, ortho, vis)
    c = T @ _sym(cov3) @ T.transpose(1, 2)
    ca = (Ta @ _sym(cov3.abs() if cov3_mag is None else cov3_mag) @ Ta.transpose(1, 2)).detach()
    a, b, d = c[:, 0, 0] + 0.3, c[:, 0, 1], c[:, 1, 1] + 0.3
    det = a * d - b * b
    mid = 0.5 * (a + d)
    lam = mid + torch.sqrt(torch.clamp_min(mid * mid - det, 0.1))
    x3 = 3.0 * torch.sqrt(lam)
    ok = vis & (det != 0) & ~torch.isnan(det)
    radius = torch.where(ok, torch.ceil(torch.nan_to_num(x3.detach(), nan=0.0, posinf=0.0)), torch.zeros_like(x3)).to(torch.int64)
    rect, q, g = tile_rect(uv[:, 0].detach(), uv[:, 1].detach(), radius.to(xyz.dtype), W, H)
    tiles = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    live = ok & (tiles != 0)
    zero = torch.zeros_like(det)
    safe = torch.where(live, det, torch.ones_like(det))
    conic = torch.stack([torch.where(live, d / safe, zero), torch.where(live, -b / safe, zero),
                         torch.where(live, a / safe, zero)], -1)
    amax = torch.maximum(ca[:, 0, 0], ca[:, 1, 1]) + 0.3
    kappa = (((ca[:, 0, 0] + 0.3) * d.abs() + a.abs() * (ca[:, 1, 1] + 0.3) + 2 * b.abs() * ca[:, 0, 1]) / det).detach()
    return dict(det=det, lam=lam, x3=x3, radius=torch.where(live, radius, 0),
                radius_raw=radius, rect=rect, rect_q=q, grid=g, tiles=torch.where(live, tiles, 0), conic=conic, live=live,
                ok=ok, abs_max=amax, kappa=kappa)


def sh_basis(dirs, deg, magnitudes=False):
    """the (deg + 1)^2 real SH basis values per row [N, nb]; ``magnitudes``: every term of every polynomial taken positive"""
    C0, C1 = 0.28209479177387814, 0.4886025119029199
    C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
    C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
          1.445305721320277, -0.5900435899266435]
    m = -1.0
    if magnitudes:
        dirs, C2, C3, m = dirs.abs(), [abs(c) for c in C2], [abs(c) for c in C3], 1.0
    x, y, z = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    B = [torch.full_like(x, C0)]
    if deg > 0:
        B += [m * C1 * y, C1 * z, m * C1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        B += [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz + m * xx + m * yy), C2[3] * xz, C2[4] * (xx + m * yy)]
    if deg > 2:
        B += [C3[0] * y * (3 * xx + m * yy), C3[1] * xy * z, C3[2] * y * (4 * zz + m * xx + m * yy),
              C3[3] * z * (2 * zz + m * 3 * xx + m * 3 * yy), C3[4] * x * (4 * zz + m * xx + m * yy), C3[5] * z * (xx + m * yy),
              C3[6] * x * (xx + m * 3 * yy)]
    return torch.stack(B, -1)


def sh_full(shs, deg, dirs, visible, free):
    """colour [N,3] (zero on invisible rows), its value before the clamp, and the magnitude its float32 rounding scales with"""
    nb = (deg + 1) ** 2
    raw = (sh_basis(dirs, deg)[:, :, None] * shs[:, :nb]).sum(1)
    mag = (sh_basis(dirs, deg, True)[:, :, None] * shs[:, :nb].abs()).sum(1)
    if not free:
        raw, mag = raw + 0.5, mag + 0.5
    col = raw if free else torch.clamp_min(raw, 0.0)
    vis = visible.reshape(-1, 1).to(col.dtype)
    return dict(color=col * vis, raw=raw, mag=mag)


# ------------------------------------------------------------------ dynamic evaluation (float64)
GAUSSIAN_MAJOR, SEGMENT_MAJOR = 0, 1


def dyn_position(position, cubic, seg, d, I, layout=GAUSSIAN_MAJOR):
    """position + cubic segment c3 + c2 d + c1 d^2 + c0 d^3; table [N,4,I,3] (Gaussian-major) or [I,N,4,3]"""
    N = position.shape[0]
    c = cubic.reshape(N, 4, I, 3)[:, :, seg] if layout == GAUSSIAN_MAJOR else cubic.reshape(I, N, 4, 3)[seg]
    return position + c[:, 3] + c[:, 2] * d + c[:, 1] * d ** 2 + c[:, 0] * d ** 3


def dyn_rotation(rotation, rot_poly, rot_fourier, basis):
    """normalize(rotation + polynomial + Fourier sums), the sums detached, the norm clamped at 1e-12 (F.normalize)"""
    N = rotation.shape[0]
    sp = (rot_poly.reshape(N, 4, 4) * basis[:4].reshape(1, 4, 1)).sum(1)
    sf = (rot_fourier.reshape(N, 8, 4) * basis[4:].reshape(1, 8, 1)).sum(1)
    q = rotation + sp.detach() + sf.detach()
    return q / torch.clamp_min(q.norm(dim=1, keepdim=True), 1e-12)


def dyn_opacity(opacity):
    return torch.sigmoid(opacity)


def dyn_scaling(scaling):
    return torch.exp(scaling)


def position_poly_fourier(position, pos_poly, pos_fourier, basis):
    N = position.shape[0]
    return position + (pos_poly.reshape(N, 4, 3) * basis[:4].reshape(1, 4, 1)).sum(1) + \
        (pos_fourier.reshape(N, 8, 3) * basis[4:].reshape(1, 8, 1)).sum(1)
