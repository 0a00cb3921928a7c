"""Seeded hard cases for the per-Gaussian geometry and the helpers that hold float32 results to the float64 twin
(tests/torch_twin.py).  Shared by tests/test_geometry_ref_cpu.py (the float32 C oracle), tests/test_gpu_geometry_reference.py
(the HIP kernels) and tools/geometry_reference_report.py.

Bars (all per Gaussian row, no outlier budget):
  uv, depth            rtol 1e-5 / atol 1e-4 px; rtol 1e-6 / atol 1e-6                  (test_pointwise_ops)
  cov3d                |a-b| <= 1e-5 |b| + 1e-6 rowmax|b|
  conic                |a-b| <= 2e-4 |b| + 1e-4 rowmax|b|
  SH colour            |a-b| <= 1e-5 |b| + 2e-6 max(rowmax|b|, 1)
  dynamic outputs      |a-b| <= 3e-6 |b| + 3e-6 rowmax|b|                                (tests/test_gpu_dynamic.py, per row)
  gradients            |a-b| <= 2e-3 |b| + 1e-4 rowscale,  rowscale = max(rowmax|b|, |g_row| * |J_row|_F) with J the
                       float64 Jacobian of the row's forward map (the natural size of a gradient that cancels); through
                       the chain cov3d -> conic the product of the two stages' norms, for the sigmoid its largest slope
  dL/dintr, dL/dextr   sums over rows: 2e-3 |b| + 1e-4 max|b| of the tensor
Rows whose float64 conditioning ``kappa`` (torch_twin.ewa_full) exceeds KAPPA0 get the conic bar and the bars of gradients
that pass through the conic multiplied by WIDEN_SLOPE * kappa / KAPPA0; the slope is 4 x the float32 C oracle's measured
envelope (profiles/geometry_reference_cpu_float32.json, checked by test_geometry_ref_cpu.py).

Decisions: a row leaves the comparison of one decision (and of what depends on it) only when its float64 distance to
that decision is within MULT * 2^-24 * (the sum of magnitudes the compared quantity is formed from).
"""
from __future__ import annotations

import math

import numpy as np
import torch

import torch_twin as tw

EPS32 = 2.0 ** -24
CULL_MULT = 16.0        # a 4-term dot product, scale, shift (and a divide on the pinhole path): <= 8 roundings; x2 for FMA / order
RADIUS_MULT = 16.0      # 16 * 2^-24 = 0.95e-6 relative: about 7x the worst float32 flip seen on the CPU (1.5e-7 from an integer)
FLOOR_MULT = 16.0
SH_MULT = 16.0
KAPPA_DEAD = 1.0 / (16.0 * EPS32)   # beyond this float32 cannot tell det from 0: the row counts as sitting on det == 0
# conditioning threshold: the float32 oracle's error on the conic grows like 4.4 * 2^-24 * kappa (envelope 0.356 of the 2e-4
# bar per 720), so up to here it stays inside the plain bar: 4.4 * 2^-24 * 720 = 1.9e-4
KAPPA0 = 720.0
WIDEN_SLOPE = 1.43      # 4 x the float32 C oracle's envelope 0.3564 (profiles/geometry_reference_cpu_float32.json)
EXCLUDE_CAP = 0.01
NEAR = {True: 0.01, False: 0.2}
EXTENT = 1.3

STRATA = ["control", "moderate", "iso", "qnorm", "thin", "edge"]
CASES = [dict(id="o1", ortho=True, N=1, W=1, H=1), dict(id="p1", ortho=False, N=1, W=1, H=1),
         dict(id="o257", ortho=True, N=257, W=17, H=33), dict(id="p257", ortho=False, N=257, W=17, H=33),
         dict(id="o3001", ortho=True, N=3001, W=854, H=480), dict(id="p3001", ortho=False, N=3001, W=854, H=480),
         dict(id="o100003", ortho=True, N=100003, W=854, H=480), dict(id="p100003", ortho=False, N=100003, W=854, H=480)]
CASE_IDS = [c["id"] for c in CASES]


def case_by_id(cid):
    return make_case(**next(c for c in CASES if c["id"] == cid))


def T64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _logu(rng, lo, hi, size):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), size=size))


def camera(W, H, ortho, frame=0):
    """``frame`` > 0: the camera of a later frame of a batch (turned a little further, shifted, another focal length)"""
    extr = np.eye(4)
    # All three axes are rotated.  The tilt out of the image plane is what float32 leaves room for under the uv bar of
    # 1e-4 px: the rounding of u is about 3 * 2^-24 * (W / 2) * sum|terms of tx| on the orthographic path, and at depth 50
    # the term e2 * z alone is 50 * sin(tilt); at W = 854 the bar allows a sum of about 1.3.  On the pinhole path the sum is
    # divided by tz, which allows a tilt ten times larger.  The small images leave 50 times more room: there the
    # orthographic camera tilts by 0.31 / -0.23 rad, so that every off-diagonal element of the rotation is of order 0.2.
    k = float(frame)
    tilt = (0.31, -0.23) if W <= 64 else (0.006, -0.005)
    extr[:3, :3] = _rot(tilt[0], tilt[1], 0.2 + 0.04 * k) if ortho else _rot(0.05 - 0.01 * k, -0.04, 0.2 + 0.04 * k)
    extr[:3, 3] = [0.11 - 0.02 * k, -0.07, 0.4 + 0.1 * k] if ortho else [0.1, -0.05 + 0.03 * k, 0.2 + 0.1 * k]
    intr = np.array([0.55 * W, 0.71 * W, 0.49 * W, 0.53 * H]) * np.array([1 + 0.03 * k, 1 - 0.02 * k, 1.0, 1.0])
    return intr.astype(np.float32), extr.astype(np.float32)


def _world(cam, extr):
    e = extr.astype(np.float64)
    return (cam - e[:3, 3]) @ e[:3, :3]          # R^T (cam - T), row vectors


def _cam_from_uvd(u, v, d, W, H, intr, ortho):
    if ortho:
        return np.stack([(u + 0.5) * 2.0 / W - 1.0, (v + 0.5) * 2.0 / H - 1.0, d], -1)
    return np.stack([(u + 0.5 - intr[2]) * d / intr[0], (v + 0.5 - intr[3]) * d / intr[1], d], -1)


def make_case(id, ortho, N, W, H, seed=0):
    """one scene: rows [0, n_edge) are the deliberate rows (near each cull bound on both sides, behind the camera, tz == 0,
    non-finite positions on the orthographic path), the rest is split evenly into the strata control / moderate / iso /
    qnorm / thin"""
    rng = np.random.default_rng(1000 + seed + N + (7 if ortho else 0))
    intr, extr = camera(W, H, ortho)
    near = NEAR[ortho]
    xlo, xhi, ylo, yhi = tw.cull_bounds(W, H, EXTENT, ortho)
    stratum = np.zeros(N, np.int64)
    # ---- bulk positions in camera space: image plane a little beyond the extent bounds, depth log-uniform to 50
    u = rng.uniform(xlo - 0.02 * (xhi - xlo), xhi + 0.02 * (xhi - xlo), N)
    v = rng.uniform(ylo - 0.02 * (yhi - ylo), yhi + 0.02 * (yhi - ylo), N)
    d = _logu(rng, near * 1.001, 50.0, N)
    cam = _cam_from_uvd(u, v, d, W, H, intr.astype(np.float64), ortho)
    edge_kind = np.full(N, "", dtype=object)
    n_edge = 0
    if N >= 64:
        uc, vc, dc = 0.45 * W, 0.55 * H, 3.0
        rows = []
        for bound in ("near", "ulo", "uhi", "vlo", "vhi"):
            for side in (-1.0, 1.0):
                for k in (4.0, 16.0, 48.0):
                    rows.append((bound, side * k))
        base = []
        for bound, _ in rows:
            uu, vv, dd = uc, vc, dc
            if bound == "near": dd = near
            if bound == "ulo": uu = xlo
            if bound == "uhi": uu = xhi
            if bound == "vlo": vv = ylo
            if bound == "vhi": vv = yhi
            base.append((uu, vv, dd))
        base = np.array(base)
        c0 = _cam_from_uvd(base[:, 0], base[:, 1], base[:, 2], W, H, intr.astype(np.float64), ortho)
        p = tw.project_full(T64(_world(c0, extr).astype(np.float32)), T64(intr), T64(extr), W, H, near, EXTENT, ortho)
        for i, (bound, k) in enumerate(rows):
            step = k * CULL_MULT * EPS32 * float(p["mag"][bound][i])
            sign = -1.0 if bound in ("uhi", "vhi") else 1.0       # dist = bound - value there
            if bound == "near": base[i, 2] += step
            if bound in ("ulo", "uhi"): base[i, 0] += sign * step
            if bound in ("vlo", "vhi"): base[i, 1] += sign * step
        ce = _cam_from_uvd(base[:, 0], base[:, 1], base[:, 2], W, H, intr.astype(np.float64), ortho)
        extra = [[0.0, 0.0, -1.0], [0.3, -0.2, -25.0], [0.1, 0.1, 0.0]]                  # behind the camera, tz == 0
        ce = np.concatenate([ce, np.array(extra)])
        kinds = [b for b, _ in rows] + ["behind", "behind", "tz0"]
        n_edge = ce.shape[0]
        cam[:n_edge] = ce
        edge_kind[:n_edge] = kinds
        stratum[:n_edge] = STRATA.index("edge")
    xyz = _world(cam, extr).astype(np.float32)
    if ortho and N >= 64:
        bad = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [-np.inf, 0, 0], [0, 0, np.nan], [0, 0, np.inf], [0, 0, -np.inf]],
                       np.float32)
        xyz[n_edge:n_edge + 6] = bad
        edge_kind[n_edge:n_edge + 6] = "nonfinite"
        stratum[n_edge:n_edge + 6] = STRATA.index("edge")
        n_edge += 6
    # ---- strata of the bulk
    nb = N - n_edge
    bulk = np.arange(n_edge, N)
    # four equal blocks and a smaller one for the thin stratum (5 %): nearly half of its rows are ill-conditioned
    sid = np.minimum((np.arange(nb) * 400) // (95 * max(nb, 1)), 4)
    stratum[bulk] = sid if N > 1 else 0
    px = np.empty((N, 3)); q = rng.normal(size=(N, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    s = stratum
    px[:] = np.exp(rng.normal(math.log(2.0), 0.5, size=(N, 3)))                    # control (and the edge rows)
    m = s == 1
    px[m] = _logu(rng, 0.05, 40.0, (m.sum(), 1)) * _logu(rng, 1.0, 30.0, (m.sum(), 3))
    m = s == 2
    iso = _logu(rng, 0.05, 40.0, (m.sum(), 1)) * np.ones((1, 3))
    iso[1::2] *= np.array([[1.0, 1.0 + 1e-4, 1.0 - 1e-4]])
    px[m] = iso
    m = s == 3
    px[m] = _logu(rng, 0.05, 40.0, (m.sum(), 1)) * _logu(rng, 1.0, 30.0, (m.sum(), 3))
    q[m] *= _logu(rng, 0.5, 2.0, (m.sum(), 1))
    m = s == 4
    px[m] = _logu(rng, 0.05, 40.0, (m.sum(), 1)) * _logu(rng, 1.0, 300.0, (m.sum(), 3))
    q[m] *= _logu(rng, 0.5, 2.0, (m.sum(), 1))
    depth = np.abs(cam[:, 2:3]) + 1e-3
    scale = px * (2.0 / W) if ortho else px * depth / float(intr[0])
    scale = scale.astype(np.float32)
    if (s == 2).any():                           # exactly isotropic after the cast
        rows_iso = np.nonzero(s == 2)[0][0::2]
        scale[rows_iso] = scale[rows_iso, :1]
    offset = (rng.normal(0, 0.02, size=(N, 3)) * (depth if not ortho else 1.0)).astype(np.float32)
    offset[:n_edge] = 0.0                        # the deliberate rows stay where they were put
    g_uv = rng.normal(size=(N, 2)).astype(np.float32)
    g_uv[np.arange(N) % 5 == 3] = 0.0            # every fifth row: a depth-only upstream gradient, so that the depth terms of
    #                                              the projection's backward are not hidden behind W / 2 times dL/duv
    return dict(id=id, ortho=ortho, N=N, W=W, H=H, intr=intr, extr=extr, xyz=xyz, scale=scale, quat=q.astype(np.float32),
                offset=offset, stratum=stratum, edge_kind=edge_kind, n_edge=n_edge, nearest=near, extent=EXTENT,
                g_uv=g_uv, g_d=rng.normal(size=(N, 1)).astype(np.float32),
                g_conic=rng.normal(size=(N, 3)).astype(np.float32), g_cov=rng.normal(size=(N, 6)).astype(np.float32))


# ------------------------------------------------------------------ float64 reference of one case
def row_jac_norm(out, inputs):
    """per row the Frobenius norm of d out[row] / d input[row] for every per-row input (rows are independent)"""
    acc = [torch.zeros(x.shape[0], dtype=torch.float64) for x in inputs]
    for k in range(out.shape[1]):
        gs = torch.autograd.grad(out[:, k].sum(), inputs, retain_graph=True, allow_unused=True)
        for a, g in zip(acc, gs):
            if g is not None:
                a += torch.nan_to_num(g).reshape(g.shape[0], -1).pow(2).sum(1)
    return [a.sqrt() for a in acc]


def _natural(outs_and_g, inputs):
    nat = [torch.zeros(x.shape[0], dtype=torch.float64) for x in inputs]
    for out, g in outs_and_g:
        gn = g.reshape(g.shape[0], -1).norm(dim=1)
        for n, j in zip(nat, row_jac_norm(out, inputs)):
            n += gn * j
    return nat


def _safe(dist, mag, mult):
    """non-finite rows are no close call: inf compares exactly and NaN propagates the same way in any precision"""
    return (dist.abs() > mult * EPS32 * mag) | ~torch.isfinite(mag) | torch.isnan(dist)


def cull_safety(p):
    """(rows whose cull flag float32 must reproduce, per bound the rows that bound leaves out): a row is a close call of a
    bound only when it lies inside that bound's margin and no other bound culls it beyond doubt"""
    raw = {k: _safe(d.detach(), p["mag"][k].detach(), CULL_MULT) for k, d in p["dist"].items()}
    sure = {k: raw[k] & ~(p["dist"][k].detach() > 0) for k in raw}              # culled by k, safely
    n = p["cull"].shape[0]
    per, safe = {}, torch.ones(n, dtype=torch.bool)
    for k in raw:
        other = torch.zeros(n, dtype=torch.bool)
        for j in raw:
            if j != k:
                other |= sure[j]
        per[k] = raw[k] | other
        safe &= per[k]
    return safe, per


def project_ref(c, xyz=None):
    """float64 projection of the case: outputs, gradients for the case's upstream gradients, decisions"""
    ortho = c["ortho"]
    x = T64(c["xyz"] if xyz is None else xyz).requires_grad_(True)
    intr = T64(c["intr"]).requires_grad_(True); extr = T64(c["extr"][:3, :4]).requires_grad_(True)
    p = tw.project_full(x, intr, extr, c["W"], c["H"], c["nearest"], c["extent"], ortho)
    safe, per = cull_safety(p)
    g_uv, g_d = T64(c["g_uv"]), T64(c["g_d"])
    nat, = _natural([(p["uv"], g_uv), (p["depth"], g_d)], [x])
    loss = (torch.nan_to_num(p["uv"]) * g_uv).sum() + (torch.nan_to_num(p["depth"]) * g_d).sum()
    dx, di, de = torch.autograd.grad(loss, [x, intr, extr], allow_unused=True)
    return dict(uv=p["uv"].detach(), depth=p["depth"].detach(), cull=p["cull"], safe=safe, safe_per=per,
                dist={k: v.detach() for k, v in p["dist"].items()}, mag={k: v.detach() for k, v in p["mag"].items()},
                dxyz=dx, dintr=di, dextr=de, nat_xyz=nat, mag_u=p["mag_u"].detach(), mag_v=p["mag_v"].detach())


def cov3d_ref(c, visible):
    s = T64(c["scale"]).requires_grad_(True); q = T64(c["quat"]).requires_grad_(True)
    cov = tw.cov3d(s, q, visible)
    g = T64(c["g_cov"])
    ns, nq = _natural([(cov, g)], [s, q])
    ds, dq = torch.autograd.grad((cov * g).sum(), [s, q])
    return dict(cov=cov.detach(), dscale=ds, dquat=dq, nat_scale=ns, nat_quat=nq)


def ewa_decisions(e, mag_u, mag_v):
    """per-row masks: ``dead`` (float32 cannot tell det from 0), ``ceil`` / ``floor`` safe"""
    dead = ~(e["kappa"] < KAPPA_DEAD) & e["ok"]
    x3 = e["x3"].detach()
    dist = torch.minimum(x3 - torch.floor(x3), torch.ceil(x3) - x3)
    ceil_safe = dist > RADIUS_MULT * EPS32 * torch.clamp_min(e["abs_max"] / e["lam"].detach(), 1.0) * x3
    q, g = e["rect_q"], e["grid"]
    r = e["radius_raw"].to(torch.float64)
    mag = torch.stack([mag_u + r, mag_v + r, mag_u + r + tw.TILE, mag_v + r + tw.TILE], -1) / tw.TILE
    near_int = torch.round(q)
    decisive = (near_int >= 1) & (near_int <= g)
    floor_safe = (~decisive | ((q - near_int).abs() > FLOOR_MULT * EPS32 * mag)).all(1)
    return dict(dead=dead, ceil_safe=ceil_safe | ~e["ok"], floor_safe=floor_safe | ~e["ok"])


def ewa_ref(c, xyz, cov3_in, uv_in, visible, g_conic=None):
    """float64 EWA projection of given (float32-valued) inputs; ``g_conic``: upstream gradient (default: the case's)"""
    ortho = c["ortho"]
    x = T64(xyz).requires_grad_(True); cov = T64(cov3_in).requires_grad_(True)
    intr = T64(c["intr"]).requires_grad_(True); extr = T64(c["extr"][:3, :4]).requires_grad_(True)
    e = tw.ewa_full(x, cov, intr, extr, T64(uv_in), c["W"], c["H"], visible, ortho)
    g = T64(c["g_conic"] if g_conic is None else g_conic)
    nx, ncov = _natural([(e["conic"], g)], [x, cov])
    dx, dcov, di, de = torch.autograd.grad((e["conic"] * g).sum(), [x, cov, intr, extr], allow_unused=True)
    out = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in e.items()}
    out.update(dxyz=dx if dx is not None else torch.zeros_like(x), dcov=dcov, dintr=di, dextr=de, nat_xyz=nx, nat_cov=ncov)
    return out


def chain_ref(c, offset=False, dyn=None):
    """float64 project -> cov3d -> EWA of the case (the fused operators), gradients of the case's upstream gradients.
    ``dyn`` = (time, table layout): position, scale and rotation come from the dynamic evaluation of the case's dynamic
    parameters (dynamics.frame_preprocess, FrameBatch.render_dynamic) and the gradients go to those parameters."""
    ortho = c["ortho"]
    if dyn is None:
        x0 = T64(c["xyz"]).requires_grad_(True)
        x = x0 + T64(c["offset"]) if offset else x0 + 0.0
        s = T64(c["scale"]).requires_grad_(True); q = T64(c["quat"]).requires_grad_(True)
        wrt = dict(dxyz=x0, dscale=s, dquat=q)
    else:
        t, layout = dyn
        seg, d, basis = _basis64(c["clock"], t)
        N, I = c["N"], c["I"]
        L = {k: T64(c[k]).requires_grad_(True) for k in ("position", "rotation", "opacity", "scaling")}
        cub = T64(c["cubic"]).reshape(N, 4, I, 3)
        cub = (cub.permute(2, 0, 1, 3).contiguous() if layout == tw.SEGMENT_MAJOR else cub).requires_grad_(True)
        x = tw.dyn_position(L["position"], cub, seg, d, I, layout)
        q = tw.dyn_rotation(L["rotation"], T64(c["rot_poly"]), T64(c["rot_fourier"]), basis)
        s, opa = tw.dyn_scaling(L["scaling"]), tw.dyn_opacity(L["opacity"])
        wrt = dict(d_position=L["position"], d_cubic=cub, d_rotation=L["rotation"], d_opacity=L["opacity"], d_scaling=L["scaling"])
    intr, extr = T64(c["intr"]), T64(c["extr"][:3, :4])
    p = tw.project_full(x, intr, extr, c["W"], c["H"], c["nearest"], c["extent"], ortho)
    vis = ~p["cull"]
    cov = tw.cov3d(s, q, vis)
    e = tw.ewa_full(x, cov, intr, extr, p["uv"], c["W"], c["H"], vis, ortho, tw.cov3d_abs(s.detach(), q.detach()))
    g_uv, g_d, g_c = T64(c["g_uv"]), T64(c["g_d"]), T64(c["g_conic"])
    # natural scale of a row's gradient: |g| times a bound of the forward Jacobian.  For scale and quaternion the bound is
    # the product of the two stages' norms (conic <- cov3d, cov3d <- parameter), which is how float32 forms the gradient:
    # the intermediate dL/dcov3d can be far larger than what survives its contraction with d cov3d / d parameter
    nx, = _natural([(p["uv"], g_uv), (p["depth"], g_d), (e["conic"], g_c)], [x])
    jc, = row_jac_norm(e["conic"], [cov])
    js, jq = row_jac_norm(cov, [s, q])
    gn = g_c.norm(dim=1)
    ns, nq = gn * jc * js, gn * jc * jq
    loss = (torch.nan_to_num(p["uv"]) * g_uv).sum() + (torch.nan_to_num(p["depth"]) * g_d).sum() + (e["conic"] * g_c).sum()
    out = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in e.items()}
    if dyn is None:
        out.update(nat_xyz=nx, nat_scale=ns, nat_quat=nq)
    else:
        g_o = T64(c["g_opa"])
        loss = loss + (opa * g_o).sum()
        jr, = row_jac_norm(q, [L["rotation"]])
        jsc, = row_jac_norm(s, [L["scaling"]])
        out.update(opa=opa.detach(), nat=dict(d_position=nx, d_cubic=nx * math.sqrt(1 + d ** 2 + d ** 4 + d ** 6),
                                              d_rotation=nq * jr, d_opacity=g_o.abs().reshape(-1) * 0.25, d_scaling=ns * jsc))
    grads = torch.autograd.grad(loss, list(wrt.values()))
    for k, gk in zip(wrt, grads):
        out[k] = gk
    if dyn is not None:
        dc = out["d_cubic"]
        out["d_cubic"] = (dc.permute(1, 2, 0, 3) if dyn[1] == tw.SEGMENT_MAJOR else dc).reshape(c["N"], -1)
    safe, _ = cull_safety(p)
    out.update(uv=p["uv"].detach(), depth=p["depth"].detach(), cull=p["cull"], cull_safe=safe,
               mag_u=p["mag_u"].detach(), mag_v=p["mag_v"].detach())
    return out


# ------------------------------------------------------------------ comparison
def widen(kappa):
    k = torch.nan_to_num(kappa, nan=0.0, posinf=KAPPA_DEAD)
    return torch.where(k > KAPPA0, torch.clamp_min(WIDEN_SLOPE * k / KAPPA0, 1.0), torch.ones_like(k))


class Report:
    """collects, per quantity and stratum, the worst error as a fraction of its bar; ``finish`` asserts"""

    def __init__(self, case):
        self.case = case
        self.worst = {}
        self.envelope = {}
        self.fail = []

    def _rows(self, rows):
        n = self.case["N"]
        return torch.ones(n, dtype=torch.bool) if rows is None else rows

    def close(self, name, got, ref, bar, rows=None):
        got = T64(np.asarray(got, np.float64)).reshape(ref.shape)
        rows = self._rows(rows)
        err = (got - ref).abs()
        same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
        ratio = torch.where(same, torch.zeros_like(err), err / torch.clamp_min(bar, 1e-300))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        ratio = ratio.reshape(ratio.shape[0], -1).max(1).values
        ratio = torch.where(rows, ratio, torch.zeros_like(ratio))
        st = torch.tensor(self.case["stratum"])
        for i, sname in enumerate(STRATA):
            m = st == i
            if m.any():
                w = float(ratio[m].max())
                self.worst[(name, sname)] = max(self.worst.get((name, sname), 0.0), w)
        nbad = int((ratio > 1).sum())
        if nbad:
            i = int(ratio.argmax())
            self.fail.append(f"{name}: {nbad} rows over the bar, worst {float(ratio[i]):.3g}x at row {i} "
                             f"({STRATA[int(st[i])]}) got {got[i].tolist()} want {ref[i].tolist()}")
        return ratio

    def equal(self, name, got, ref, rows=None):
        got = torch.as_tensor(np.asarray(got)).reshape(ref.shape).to(ref.dtype)
        rows = self._rows(rows)
        bad = (got != ref) & rows
        self.worst[(name, "all")] = max(self.worst.get((name, "all"), 0.0), float(bad.sum()))
        if bad.any():
            i = int(torch.nonzero(bad)[0])
            self.fail.append(f"{name}: {int(bad.sum())} rows differ, first row {i} ({STRATA[int(self.case['stratum'][i])]}) "
                             f"got {got[i].tolist()} want {ref[i].tolist()}")

    def tensor(self, name, got, ref):
        """a sum over rows (dL/dintr, dL/dextr): relative to the tensor's maximum"""
        got = T64(np.asarray(got, np.float64)).reshape(-1)[:ref.numel()].reshape(ref.shape)
        bar = 2e-3 * ref.abs() + 1e-4 * ref.abs().max()
        w = float(((got - ref).abs() / torch.clamp_min(bar, 1e-300)).max())
        self.worst[(name, "all")] = max(self.worst.get((name, "all"), 0.0), w)
        if w > 1:
            self.fail.append(f"{name}: {w:.3g}x the bar, got {got.tolist()} want {ref.tolist()}")

    def lines(self):
        return [f"{self.case['id']:>8} {k[0]:<22} {k[1]:<9} {v:.3g}" for k, v in sorted(self.worst.items())]

    def finish(self):
        print("\n".join(self.lines()))
        assert not self.fail, "\n".join(self.fail)


def value_bar(ref, rtol, frac, floor=0.0):
    rm = ref.abs().reshape(ref.shape[0], -1).max(1).values.clamp_min(floor)
    return rtol * ref.abs() + frac * rm.reshape(-1, *([1] * (ref.dim() - 1)))


def grad_bar(ref, nat):
    rm = torch.maximum(torch.nan_to_num(ref).abs().reshape(ref.shape[0], -1).max(1).values, nat)
    return 2e-3 * ref.abs() + 1e-4 * rm.reshape(-1, *([1] * (ref.dim() - 1)))


def uv_bar(ref):
    return 1e-5 * ref.abs() + 1e-4


def depth_bar(ref):
    return 1e-6 * ref.abs() + 1e-6


def check_project(rep, tag, r, uv, depth, dxyz=None, dintr=None, dextr=None):
    """r = project_ref(...)"""
    s = r["safe"]
    rep.equal(tag + "cull", np.asarray(depth).reshape(-1) == 0, r["cull"] | (r["depth"].reshape(-1) == 0), s)
    rep.close(tag + "uv", uv, r["uv"], uv_bar(r["uv"]), s)
    rep.close(tag + "depth", depth, r["depth"], depth_bar(r["depth"]), s)
    if dxyz is not None:
        rep.close(tag + "dL_dxyz", dxyz, r["dxyz"], grad_bar(r["dxyz"], r["nat_xyz"]), s)
    if dintr is not None:
        rep.tensor(tag + "dL_dintr", dintr, r["dintr"])
    if dextr is not None:
        rep.tensor(tag + "dL_dextr", dextr, r["dextr"])


def check_cov3d(rep, tag, r, cov, dscale=None, dquat=None):
    rep.close(tag + "cov3d", cov, r["cov"], value_bar(r["cov"], 1e-5, 1e-6))
    if dscale is not None:
        rep.close(tag + "dL_dscale", dscale, r["dscale"], grad_bar(r["dscale"], r["nat_scale"]))
        rep.close(tag + "dL_dquat", dquat, r["dquat"], grad_bar(r["dquat"], r["nat_quat"]))


def ewa_rows(e, mag_u, mag_v, base=None):
    """row masks of one EWA reference: which rows take part in the radius / tiles / conic comparisons"""
    d = ewa_decisions(e, mag_u, mag_v)
    n = e["det"].shape[0]
    base = torch.ones(n, dtype=torch.bool) if base is None else base
    r_rows = base & ~d["dead"] & d["ceil_safe"] & d["floor_safe"]     # radius is 0 for an empty rectangle: needs the floors too
    return d, r_rows


def check_ewa(rep, tag, e, rows, conic, radius, tiles, grads=()):
    """grads: (name, got, ref, natural, through): the bar of a gradient that passes through the conic (``through``) widens
    with the row's conditioning like the conic's own; the others keep the plain bar"""
    w = widen(e["kappa"])[:, None]
    ill = (e["kappa"] > KAPPA0) & rows & e["live"]
    rep.equal(tag + "radius", radius, e["radius"], rows)
    if tiles is not None:
        rep.equal(tag + "tiles", tiles, e["tiles"], rows)
    todo = [("conic", conic, e["conic"], value_bar(e["conic"], 2e-4, 1e-4), True)]
    todo += [(name, got, ref, grad_bar(ref, nat), through) for name, got, ref, nat, through in grads]
    for name, got, ref, bar, through in todo:
        if not through:
            rep.close(tag + name, got, ref, bar, rows)
            continue
        ratio = rep.close(tag + name, got, ref, bar * w, rows)
        # what the slope of the widening is calibrated from: the error of the ill-conditioned rows as a fraction of the
        # PLAIN bar, per unit of kappa / KAPPA0
        env = float((ratio * w[:, 0] / (e["kappa"] / KAPPA0))[ill].max()) if ill.any() else 0.0
        rep.envelope[tag + name] = max(rep.envelope.get(tag + name, 0.0), env)


def exclusion_counts(c, masks):
    """{decision: (excluded in the bulk, bulk rows, excluded among the deliberate rows, deliberate rows)}"""
    edge = torch.tensor(c["stratum"] == STRATA.index("edge"))
    return {k: (int((~m & ~edge).sum()), int((~edge).sum()), int((~m & edge).sum()), int(edge.sum())) for k, m in masks.items()}


def assert_caps(c, masks):
    """at most 1 % of the rows per decision.  The deliberate rows are counted on their own for the cull bounds they were
    placed at; for the EWA decisions they are rows like any other."""
    for k, (xb, nb, xe, ne) in exclusion_counts(c, masks).items():
        if k in ("det", "ceil", "floor"):
            assert xb + xe <= int(EXCLUDE_CAP * (nb + ne)), f"{c['id']}: decision {k} leaves out {xb + xe} of {nb + ne} rows"
            continue
        assert xb <= int(EXCLUDE_CAP * nb), f"{c['id']}: decision {k} leaves out {xb} of {nb} bulk rows"
        assert xe <= int(EXCLUDE_CAP * ne), f"{c['id']}: decision {k} leaves out {xe} of {ne} deliberate rows"


def assert_bounds_populated(c, r):
    """the deliberate rows put both sides of every cull bound just outside the margin"""
    if not c["n_edge"]:
        return
    for kind in ("behind", "tz0", "nonfinite"):          # and these rows are culled, whatever the precision
        sel = torch.tensor(c["edge_kind"] == kind)
        assert bool(r["cull"][sel].all()) and bool(r["safe"][sel].all()), f"{c['id']}: a {kind} row is not culled beyond doubt"
    for k, dist in r["dist"].items():
        m = CULL_MULT * EPS32 * r["mag"][k]
        sel = torch.tensor(c["edge_kind"] == k)
        for sign in (-1.0, 1.0):
            hit = sel & (sign * dist > m) & (sign * dist < 100 * m)
            assert hit.any(), f"{c['id']}: no row just {'inside' if sign > 0 else 'outside'} bound {k}"


# ------------------------------------------------------------------ one case through a backend
# A backend runs the float32 code under test and returns numpy arrays:
#   project(c, xyz, g_uv, g_d)            -> uv, depth, dxyz, dintr, dextr        (dintr / dextr None on the orthographic path)
#   cov3d(c, scale, quat, vis, g)         -> cov, dscale, dquat
#   ewa(c, xyz, cov3, uv, vis, g)         -> conic, radius, tiles, dxyz, dcov, dintr, dextr
#   fused(c, offset)                      -> uv, depth, conic, radius, tiles, dxyz, dscale, dquat
def run_operators(backend, c, rep):
    """project_point, compute_cov3d and ewa_project one by one, each fed float32 roundings of the float64 upstream results;
    returns the decision masks (for the exclusion caps)"""
    r = project_ref(c)
    b = backend.project(c, c["xyz"], c["g_uv"], c["g_d"])
    check_project(rep, "project.", r, b["uv"], b["depth"], b["dxyz"], b.get("dintr"), b.get("dextr"))
    vis = ~r["cull"]
    cr = cov3d_ref(c, vis)
    b = backend.cov3d(c, c["scale"], c["quat"], vis.numpy(), c["g_cov"])
    check_cov3d(rep, "cov3d.", cr, b["cov"], b["dscale"], b["dquat"])
    cov_in = cr["cov"].numpy().astype(np.float32)
    uv_in = np.nan_to_num(r["uv"].numpy()).astype(np.float32)
    e = ewa_ref(c, np.nan_to_num(c["xyz"], posinf=0.0, neginf=0.0), cov_in, uv_in, vis)
    d, rows = ewa_rows(e, r["mag_u"], r["mag_v"])
    b = backend.ewa(c, c["xyz"], cov_in, uv_in, vis.numpy(), c["g_conic"])
    grads = [("dL_dcov3d", b["dcov"], e["dcov"], e["nat_cov"], True)]
    if not c["ortho"]:
        grads.append(("dL_dxyz", b["dxyz"], e["dxyz"], e["nat_xyz"], True))
    check_ewa(rep, "ewa.", e, rows, b["conic"], b["radius"], b["tiles"], grads)
    if not c["ortho"]:
        # the camera gradients are sums over rows and keep the tensor bar: a second backward pass whose upstream gradient is
        # zero, on both sides, on the rows that were left out or are ill-conditioned
        keep = (rows & ~(e["kappa"] > KAPPA0)).numpy()
        g = c["g_conic"] * keep[:, None].astype(np.float32)
        e2 = ewa_ref(c, c["xyz"], cov_in, uv_in, vis, g)
        b2 = backend.ewa(c, c["xyz"], cov_in, uv_in, vis.numpy(), g)
        rep.tensor("ewa.dL_dintr", np.asarray(b2["dintr"])[:2], e2["dintr"][:2])
        rep.tensor("ewa.dL_dextr", b2["dextr"], e2["dextr"])
    masks = dict(r["safe_per"], det=~d["dead"], ceil=d["ceil_safe"], floor=d["floor_safe"])
    return r, e, masks


def check_chain(rep, tag, r, b, grads=()):
    """the per-Gaussian results of a whole chain ``b`` (uv, depth, conic, radius, optionally tiles) against chain_ref's ``r``"""
    d, rows = ewa_rows(r, r["mag_u"], r["mag_v"], r["cull_safe"])
    s = r["cull_safe"]
    rep.equal(tag + "cull", np.asarray(b["depth"]).reshape(-1) == 0, r["cull"] | (r["depth"].reshape(-1) == 0), s)
    rep.close(tag + "uv", b["uv"], r["uv"], uv_bar(r["uv"]), s)
    rep.close(tag + "depth", b["depth"], r["depth"], depth_bar(r["depth"]), s)
    check_ewa(rep, tag, r, rows, b["conic"], b["radius"], b.get("tiles"), grads)
    return dict(det=~d["dead"], ceil=d["ceil_safe"], floor=d["floor_safe"])


def run_fused(backend, c, rep, offset, tag="fused."):
    r = chain_ref(c, offset)
    b = backend.fused(c, offset)
    # (the orthographic EWA Jacobian is constant: there the position gradient does not pass through the conic)
    r["doffset"] = r["dxyz"]
    grads = [(n, b[k], r[k], r["nat_" + m], th) for n, k, m, th in (
        ("dL_dxyz", "dxyz", "xyz", not c["ortho"]), ("dL_doffset", "doffset", "xyz", not c["ortho"]),
        ("dL_dscale", "dscale", "scale", True), ("dL_dquat", "dquat", "quat", True)) if b.get(k) is not None]
    return r, check_chain(rep, tag, r, b, grads)


def frame_cases(c, F, offsets):
    """the F per-frame variants of a case for a batch: its own camera each, and (``offsets``) a displacement that grows"""
    out = []
    for f in range(F):
        intr, extr = camera(c["W"], c["H"], c["ortho"], f)
        off = (c["offset"] * (f + 1)).astype(np.float32) if offsets else np.zeros_like(c["offset"])
        out.append(dict(c, intr=intr, extr=extr, offset=off))
    return out


def make_dyn_geom_case(cid, T=21):
    """an orthographic geometry case whose positions, scales and rotations are produced by the dynamic evaluation: base
    position = the case's, a small spline displacement, scaling logits = log(scale), rotation = the case's quaternions
    (any norm: the evaluation normalises), opacity logits including +-30"""
    c = case_by_id(cid)
    assert c["ortho"]
    d = make_dyn_case(c["N"], T)
    d["id"] = "dyn_" + cid
    d["cubic"] = (d["cubic"] * 0.1).astype(np.float32)
    d.update(position=c["xyz"], scaling=np.log(c["scale"]).astype(np.float32), rotation=c["quat"].copy(), stratum=c["stratum"])
    for k in ("W", "H", "ortho", "intr", "extr", "nearest", "extent", "g_uv", "g_d", "g_conic", "n_edge", "edge_kind"):
        d[k] = c[k]
    return d


def run_frame_preprocess(backend, c, rep, t, layout, tag="frame."):
    r = chain_ref(c, dyn=(t, layout))
    b = backend.frame_preprocess(c, t, layout)
    grads = [(k, b[k], r[k], r["nat"][k], k in ("d_rotation", "d_scaling"))
             for k in ("d_position", "d_cubic", "d_rotation", "d_scaling")]
    masks = check_chain(rep, tag, r, b, grads)
    rep.close(tag + "opa", b["opa"], r["opa"], value_bar(r["opa"], 3e-6, 3e-6))
    rep.close(tag + "d_opacity", b["d_opacity"], r["d_opacity"], grad_bar(r["d_opacity"], r["nat"]["d_opacity"]))
    return r, masks


def conditioned_share(e):
    """share of the live rows at or below the conditioning threshold"""
    live = e["live"]
    return float((e["kappa"][live] <= KAPPA0).double().mean()) if live.any() else 1.0


# ------------------------------------------------------------------ SH colour
SH_P = 4099


def make_sh_case(deg, seed=0):
    """generic and polar directions, invisible rows, and rows whose colour sits on both sides of the clamp at 0: a few
    inside the margin (within 1e-6), the others 4, 16 and 48 margins away"""
    rng = np.random.default_rng(500 + deg + seed)
    P, nb = SH_P, (deg + 1) ** 2
    shs = rng.normal(0, 0.5, size=(P, nb, 3)).astype(np.float32)
    dirs = rng.normal(size=(P, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    poles = np.array([[0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
    dirs[:P // 4] = poles[np.arange(P // 4) % 6]
    dirs = dirs.astype(np.float32)
    vis = rng.uniform(size=P) > 0.1
    near = np.arange(P // 2, P // 2 + 64)
    vis[near] = True
    steps = np.array([-48.0, -16.0, -4.0, -0.25, 0.25, 4.0, 16.0, 48.0])
    k = steps[np.arange(near.size) % 8]
    sh0 = shs.copy(); sh0[near, 0, :] = 0
    f = tw.sh_full(T64(sh0), deg, T64(dirs), torch.ones(P), False)
    margin = SH_MULT * EPS32 * (f["mag"][near] + 1.0)                  # (+1: the constant term still to be set is below 1 / C0)
    target = T64(k)[:, None] * margin
    shs[near, 0, :] = ((target - f["raw"][near]) / 0.28209479177387814).numpy().astype(np.float32)
    return dict(id=f"sh{deg}", N=P, deg=deg, shs=shs, dirs=dirs, vis=vis, near=near, stratum=np.zeros(P, np.int64),
                g=rng.normal(size=(P, 3)).astype(np.float32))


def sh_ref(c, free):
    shs = T64(c["shs"]).requires_grad_(True); dirs = T64(c["dirs"]).requires_grad_(True)
    vis = torch.tensor(c["vis"])
    f = tw.sh_full(shs, c["deg"], dirs, vis, free)
    g = T64(c["g"])
    nsh, ndir = _natural([(f["color"], g)], [shs, dirs])
    dsh, ddir = torch.autograd.grad((f["color"] * g).sum(), [shs, dirs], allow_unused=True)
    safe = torch.ones(c["N"], dtype=torch.bool)
    if not free:
        safe = (_safe(f["raw"].detach(), f["mag"].detach(), SH_MULT) | ~vis[:, None]).all(1)
    return dict(color=f["color"].detach(), raw=f["raw"].detach(), mag=f["mag"].detach(), dshs=dsh,
                ddirs=ddir if ddir is not None else torch.zeros_like(dirs), nat_shs=nsh, nat_dirs=ndir, safe=safe)


def run_sh(backend, c, rep, free):
    r = sh_ref(c, free)
    b = backend.sh(c, free)
    tag = "sh_free." if free else "sh."
    rep.close(tag + "color", b["color"], r["color"], value_bar(r["color"], 1e-5, 2e-6, floor=1.0))
    rep.close(tag + "dL_dshs", b["dshs"], r["dshs"], grad_bar(r["dshs"], r["nat_shs"]), r["safe"])
    if c["deg"] > 0:
        rep.close(tag + "dL_ddirs", b["ddirs"], r["ddirs"], grad_bar(r["ddirs"], r["nat_dirs"]), r["safe"])
    return r


def assert_sh_clamp_populated(c, r):
    """both sides of the clamp hold rows just outside the margin, and the rows inside it stay under the cap"""
    m = SH_MULT * EPS32 * r["mag"][c["near"]]
    raw = r["raw"][c["near"]]
    for sign in (-1.0, 1.0):
        assert ((sign * raw > m) & (sign * raw < 100 * m)).any(), f"{c['id']}: no colour just {'above' if sign > 0 else 'below'} the clamp"
    assert (raw.abs() < 1e-6).any(), f"{c['id']}: no colour within 1e-6 of the clamp"
    out = int((~r["safe"]).sum())
    assert out <= int(EXCLUDE_CAP * c["N"]), f"{c['id']}: the clamp leaves out {out} of {c['N']} rows"


# ------------------------------------------------------------------ dynamic evaluation
DYN_SIZES = [1, 257, 100003]


def dyn_clock(T):
    from splatter_a_video_amd.dynamics import FrameClock
    return FrameClock(T)


def make_dyn_case(N, T=21, seed=0):
    """parameters of the dynamic point cloud; with N >= 64 the first rows are deliberate: quaternion sums of norm 1e-10,
    1e-11, 1e-13 (below the 1e-12 clamp of F.normalize) and exactly 0, opacity logits +-30, scaling logits -12 .. +3.
    ``times``: the first and last frame, every spline knot and frames inside segments."""
    rng = np.random.default_rng(900 + N + seed)
    clock = dyn_clock(T)
    I = clock.interval_num
    f = lambda *s, scale=1.0: rng.normal(0, scale, size=s).astype(np.float32)
    c = dict(id=f"dyn{N}", N=N, T=T, I=I, clock=clock, stratum=np.zeros(N, np.int64),
             position=f(N, 3), cubic=f(N, 4 * I * 3, scale=0.1), rotation=f(N, 4), rot_poly=f(N, 4, 4, scale=0.05),
             rot_fourier=f(N, 8, 4, scale=0.05), opacity=f(N, 1, scale=1.5), scaling=f(N, 3, scale=0.5) - 4.0,
             pos_poly=f(N, 4, 3, scale=0.1), pos_fourier=f(N, 8, 3, scale=0.1),
             g_pos=f(N, 3), g_rot=f(N, 4), g_opa=f(N, 1), g_scl=f(N, 3))
    if N >= 64:
        c["stratum"][:10] = STRATA.index("edge")
        c["rot_poly"][:4] = 0; c["rot_fourier"][:4] = 0
        v = c["rotation"][:4].astype(np.float64); v /= np.linalg.norm(v, axis=1, keepdims=True)
        c["rotation"][:4] = (v * np.array([[1e-10], [1e-11], [1e-13], [0.0]])).astype(np.float32)
        c["opacity"][4:6, 0] = [30.0, -30.0]
        c["scaling"][6:10] = np.array([[-12, -12, -12], [3, 3, 3], [-12, 3, 0], [3, -12, -5]], np.float32)
    knots = (clock.intervals.astype(np.float64) * (T - 1)).round().astype(int).tolist()
    c["times"] = sorted(set([0, 1, T - 1, T // 2] + knots))
    return c


def _basis64(clock, t):
    seg, d, basis = clock.scalars(t)
    return seg, float(np.float32(d)), T64(np.frombuffer(basis, dtype=np.float32, count=12).copy())


def dyn_ref(c, t, layout=tw.GAUSSIAN_MAJOR):
    seg, d, basis = _basis64(c["clock"], t)
    N, I = c["N"], c["I"]
    L = {k: T64(c[k]).requires_grad_(True) for k in ("position", "rotation", "opacity", "scaling")}
    cub = T64(c["cubic"]).reshape(N, 4, I, 3)
    cub = (cub.permute(2, 0, 1, 3).contiguous() if layout == tw.SEGMENT_MAJOR else cub).requires_grad_(True)
    pos = tw.dyn_position(L["position"], cub, seg, d, I, layout)
    rot = tw.dyn_rotation(L["rotation"], T64(c["rot_poly"]), T64(c["rot_fourier"]), basis)
    opa, scl = tw.dyn_opacity(L["opacity"]), tw.dyn_scaling(L["scaling"])
    g = {k: T64(c["g_" + k]) for k in ("pos", "rot", "opa", "scl")}
    n_rot, = _natural([(rot, g["rot"])], [L["rotation"]])
    loss = (pos * g["pos"]).sum() + (rot * g["rot"]).sum() + (opa * g["opa"]).sum() + (scl * g["scl"]).sum()
    dp, dc, dr, do, ds = torch.autograd.grad(loss, [L["position"], cub, L["rotation"], L["opacity"], L["scaling"]])
    if layout == tw.SEGMENT_MAJOR:
        dc = dc.permute(1, 2, 0, 3)
    gp = g["pos"].norm(dim=1)
    return dict(pos=pos.detach(), rot=rot.detach(), opa=opa.detach(), scl=scl.detach(), d_position=dp,
                d_cubic=dc.reshape(N, -1), d_rotation=dr, d_opacity=do, d_scaling=ds,
                nat=dict(d_position=gp, d_cubic=gp * math.sqrt(1 + d ** 2 + d ** 4 + d ** 6), d_rotation=n_rot,
                         d_opacity=g["opa"].abs().reshape(-1) * 0.25,          # sup of the sigmoid's slope
                         d_scaling=(g["scl"] * scl.detach()).norm(dim=1)))


def run_dyn(backend, c, rep, t, layout=tw.GAUSSIAN_MAJOR, tag="dyn."):
    """values: rtol 3e-6 + 3e-6 of the row maximum (the existing 3e-6 of tests/test_gpu_dynamic.py, per row)"""
    r = dyn_ref(c, t, layout)
    b = backend.dyn(c, t, layout)
    for k in ("pos", "rot", "opa", "scl"):
        rep.close(tag + k, b[k], r[k], value_bar(r[k], 3e-6, 3e-6))
    for k, nat in r["nat"].items():
        rep.close(tag + k, b[k], r[k], grad_bar(r[k], nat))
    return r


def ppf_ref(c, t):
    _, _, basis = _basis64(c["clock"], t)
    L = [T64(c[k]).requires_grad_(True) for k in ("position", "pos_poly", "pos_fourier")]
    pos = tw.position_poly_fourier(L[0], L[1], L[2], basis)
    g = T64(c["g_pos"])
    dp, dpoly, dfour = torch.autograd.grad((pos * g).sum(), L)
    gn = g.norm(dim=1)
    return dict(pos=pos.detach(), d_position=dp, d_poly=dpoly, d_fourier=dfour,
                nat=dict(d_position=gn, d_poly=gn * basis[:4].norm(), d_fourier=gn * basis[4:].norm()))


def run_ppf(backend, c, rep, t, tag="ppf."):
    r = ppf_ref(c, t)
    b = backend.ppf(c, t)
    # 13 terms of mixed sign: the rounding scales with the sum of their magnitudes, not with the result
    mag = T64(c["position"]).abs() + (T64(c["pos_poly"]).abs().sum(1) + T64(c["pos_fourier"]).abs().sum(1))
    rep.close(tag + "pos", b["pos"], r["pos"], 3e-6 * r["pos"].abs() + 3e-6 * mag.max(1, keepdim=True).values)
    for k, nat in r["nat"].items():
        rep.close(tag + k, b[k], r[k], grad_bar(r[k], nat))


class OracleBackend:
    """the C oracle's operators behind the backend interface of geometry_ref.run_operators / run_fused"""

    def __init__(self, o):
        self.o = o

    def project(self, c, xyz, g_uv, g_d):
        o = self.o
        if c["ortho"]:
            uv, d = o.project_point_ortho_forward(xyz, c["extr"], c["W"], c["H"], c["nearest"], c["extent"])
            return dict(uv=uv, depth=d, dxyz=o.project_point_ortho_backward(c["extr"], c["W"], c["H"], d, g_uv, g_d))
        uv, d = o.project_point_forward(xyz, c["intr"], c["extr"], c["W"], c["H"], c["nearest"], c["extent"])
        dx, di, de = o.project_point_backward(xyz, c["intr"], c["extr"], c["W"], c["H"], uv, d, g_uv, g_d)
        return dict(uv=uv, depth=d, dxyz=dx, dintr=di, dextr=de)

    def cov3d(self, c, scale, quat, vis, g):
        ds, dq = self.o.compute_cov3d_backward(scale, quat, vis, g)
        return dict(cov=self.o.compute_cov3d_forward(scale, quat, vis), dscale=ds, dquat=dq)

    def ewa(self, c, xyz, cov3, uv, vis, g):
        o = self.o
        conic, radius, tiles = o.ewa_project_forward(xyz, cov3, c["intr"], c["extr"], uv, c["W"], c["H"], vis, ortho=c["ortho"])
        dx, dcov, di, de = o.ewa_project_backward(xyz, cov3, c["intr"], c["extr"], radius, g, c["W"], c["H"], ortho=c["ortho"])
        return dict(conic=conic, radius=radius, tiles=tiles, dxyz=dx, dcov=dcov, dintr=di, dextr=de)

    def fused(self, c, offset):
        o = self.o
        xyz = (c["xyz"] + c["offset"]).astype(np.float32) if offset else c["xyz"]
        p = self.project(c, xyz, c["g_uv"], c["g_d"])
        vis = p["depth"].reshape(-1) != 0
        cov = o.compute_cov3d_forward(c["scale"], c["quat"], vis)
        e = self.ewa(c, xyz, cov, p["uv"], vis, c["g_conic"])
        ds, dq = o.compute_cov3d_backward(c["scale"], c["quat"], vis, e["dcov"])
        return dict(uv=p["uv"], depth=p["depth"], conic=e["conic"], radius=e["radius"], tiles=e["tiles"],
                    dxyz=p["dxyz"] + e["dxyz"], dscale=ds, dquat=dq)

    def sh(self, c, free):
        o = self.o
        if free:
            col, cl = o.compute_sh_forward(c["shs"], c["deg"], c["dirs"], c["vis"], free=True), None
        else:
            col, cl = o.compute_sh_forward(c["shs"], c["deg"], c["dirs"], c["vis"])
        dsh, dd = o.compute_sh_backward(c["shs"], c["deg"], c["dirs"], c["vis"], cl, c["g"], free=free)
        return dict(color=col, dshs=dsh, ddirs=dd)

    def dyn(self, c, t, layout):
        assert layout == tw.GAUSSIAN_MAJOR, "the oracle knows the reference's table layout only"
        o = self.o
        seg, d, poly, four = o.dynamic_time_scalars(t, c["T"], c["clock"].intervals, 0, c["T"] - 1)
        pos, rot, opa, scl = o.dynamic_eval_forward(c["position"], c["cubic"], c["rotation"], c["rot_poly"], c["rot_fourier"],
                                                    c["opacity"], c["scaling"], seg, d, poly, four)
        g = o.dynamic_eval_backward((c["N"], 4, c["I"], 3), c["rotation"], c["rot_poly"], c["rot_fourier"], c["opacity"],
                                    c["scaling"], seg, d, poly, four, c["g_pos"], c["g_rot"], c["g_opa"], c["g_scl"])
        return dict(pos=pos, rot=rot, opa=opa, scl=scl, d_position=g[0], d_cubic=g[1].reshape(c["N"], -1), d_rotation=g[2],
                    d_opacity=g[3], d_scaling=g[4])

    def ppf(self, c, t):
        o = self.o
        b = o.time_basis(t, 0, c["T"] - 1)
        dp, dpoly, dfour = o.position_poly_fourier_backward(c["g_pos"], b)
        return dict(pos=o.position_poly_fourier_forward(c["position"], c["pos_poly"], c["pos_fourier"], b), d_position=dp,
                    d_poly=dpoly, d_fourier=dfour)

    def frame_preprocess(self, c, t, layout):
        """the oracle's dynamic evaluation followed by its operator chain"""
        d = self.dyn(c, t, tw.GAUSSIAN_MAJOR)
        o = self.o
        cc = dict(c, xyz=d["pos"], scale=d["scl"], quat=d["rot"])
        f = self.fused(cc, False)
        seg, dd, poly, four = o.dynamic_time_scalars(t, c["T"], c["clock"].intervals, 0, c["T"] - 1)
        g = o.dynamic_eval_backward((c["N"], 4, c["I"], 3), c["rotation"], c["rot_poly"], c["rot_fourier"], c["opacity"],
                                    c["scaling"], seg, dd, poly, four, f["dxyz"], f["dquat"], c["g_opa"], f["dscale"])
        return dict(f, opa=d["opa"], d_position=g[0], d_cubic=g[1].reshape(c["N"], -1), d_rotation=g[2], d_opacity=g[3],
                    d_scaling=g[4])


class HipBackend:
    """the HIP operators (dptr.gs surface) behind the same interface; ``sink``: the fused backward adds into caller buffers"""

    def __init__(self, device, sink=False):
        import dptr.gs as gs
        self.gs, self.dev, self.sink = gs, device, sink

    def t(self, a, grad=False):
        x = torch.as_tensor(np.ascontiguousarray(a), device=self.dev)
        return x.requires_grad_(True) if grad else x

    @staticmethod
    def n(x):
        return None if x is None else x.detach().cpu().numpy()

    def project(self, c, xyz, g_uv, g_d):
        gs = self.gs
        x = self.t(xyz, True); extr = self.t(c["extr"], not c["ortho"])
        if c["ortho"]:
            intr = None
            uv, d = gs.project_point_ortho(x, extr, c["W"], c["H"], nearest=c["nearest"], extent=c["extent"])
        else:
            intr = self.t(c["intr"], True)
            uv, d = gs.project_point(x, intr, extr, c["W"], c["H"], nearest=c["nearest"], extent=c["extent"])
        ((uv.nan_to_num() * self.t(g_uv)).sum() + (d * self.t(g_d)).sum()).backward()
        out = dict(uv=self.n(uv), depth=self.n(d), dxyz=self.n(x.grad))
        if not c["ortho"]:
            out.update(dintr=self.n(intr.grad), dextr=self.n(extr.grad)[:3, :4])
        return out

    def cov3d(self, c, scale, quat, vis, g):
        s = self.t(scale, True); q = self.t(quat, True)
        cov = self.gs.compute_cov3d(s, q, self.t(vis).reshape(-1, 1))
        (cov * self.t(g)).sum().backward()
        return dict(cov=self.n(cov), dscale=self.n(s.grad), dquat=self.n(q.grad))

    def ewa(self, c, xyz, cov3, uv, vis, g):
        gs = self.gs
        x = self.t(xyz, True); cov = self.t(cov3, True); extr = self.t(c["extr"], not c["ortho"])
        if c["ortho"]:
            intr = None
            conic, radius, tiles = gs.ewa_project_ortho(x, cov, extr, self.t(uv), c["W"], c["H"], self.t(vis))
        else:
            intr = self.t(c["intr"], True)
            conic, radius, tiles = gs.ewa_project(x, cov, intr, extr, self.t(uv), c["W"], c["H"], self.t(vis))
        (conic * self.t(g)).sum().backward()
        out = dict(conic=self.n(conic), radius=self.n(radius), tiles=self.n(tiles), dcov=self.n(cov.grad),
                   dxyz=self.n(x.grad) if x.grad is not None else np.zeros_like(xyz))
        if not c["ortho"]:
            out.update(dintr=self.n(intr.grad), dextr=self.n(extr.grad)[:3, :4])
        return out

    def fused(self, c, offset):
        gs = self.gs
        x = self.t(c["xyz"], True); s = self.t(c["scale"], True); q = self.t(c["quat"], True)
        # without a sink the offset asks for its own gradient; with one, two passes ADD into the same buffers (x + x is exact)
        off = self.t(c["offset"], not self.sink) if offset else None
        sink = {k: torch.zeros_like(v) for k, v in dict(xyz=x, scales=s, uquats=q).items()} if self.sink else None
        kw = dict(nearest=c["nearest"], extent=c["extent"], offset=off, grad_sink=sink)
        for _ in range(2 if self.sink else 1):
            if c["ortho"]:
                uv, d, conic, radius, tiles = gs.preprocess_ortho(x, s, q, self.t(c["extr"]), c["W"], c["H"], **kw)
            else:
                uv, d, conic, radius, tiles = gs.preprocess_persp(x, s, q, self.t(c["intr"]), self.t(c["extr"]), c["W"], c["H"], **kw)
            ((uv.nan_to_num() * self.t(c["g_uv"])).sum() + (d * self.t(c["g_d"])).sum() + (conic * self.t(c["g_conic"])).sum()).backward()
        if self.sink:
            assert x.grad is None and s.grad is None and q.grad is None, "a sinked input must not receive an autograd gradient"
            grads = (sink["xyz"] * 0.5, sink["scales"] * 0.5, sink["uquats"] * 0.5)
        else:
            grads = (x.grad, s.grad, q.grad)
        out = dict(uv=self.n(uv), depth=self.n(d), conic=self.n(conic), radius=self.n(radius), tiles=self.n(tiles),
                   dxyz=self.n(grads[0]), dscale=self.n(grads[1]), dquat=self.n(grads[2]))
        if off is not None and off.requires_grad:
            out["doffset"] = self.n(off.grad)
        return out

    def sh(self, c, free):
        sh = self.t(c["shs"], True); d = self.t(c["dirs"], True)
        fn = self.gs.compute_sh_free if free else self.gs.compute_sh
        col = fn(sh, c["deg"], d, self.t(c["vis"]))
        (col * self.t(c["g"])).sum().backward()
        return dict(color=self.n(col), dshs=self.n(sh.grad), ddirs=self.n(d.grad))

    def dyn(self, c, t, layout):
        from splatter_a_video_amd import dynamics as dy
        N, I = c["N"], c["I"]
        p = {k: self.t(c[k], True) for k in ("position", "rotation", "opacity", "scaling")}
        cub = self.t(c["cubic"])
        cub = (dy.to_segment_major(cub, I) if layout == tw.SEGMENT_MAJOR else cub).requires_grad_(True)
        pos, rot, opa, scl = dy.evaluate(c["clock"], t, position=p["position"], pos_cubic_node=cub, rotation=p["rotation"],
                                         rot_poly_feat=self.t(c["rot_poly"]), rot_fourier_feat=self.t(c["rot_fourier"]),
                                         opacity=p["opacity"], scaling=p["scaling"], cubic_layout=layout)
        ((pos * self.t(c["g_pos"])).sum() + (rot * self.t(c["g_rot"])).sum() + (opa * self.t(c["g_opa"])).sum()
         + (scl * self.t(c["g_scl"])).sum()).backward()
        dc = cub.grad
        dc = dy.to_gaussian_major(dc) if layout == tw.SEGMENT_MAJOR else dc.reshape(N, -1)
        return dict(pos=self.n(pos), rot=self.n(rot), opa=self.n(opa), scl=self.n(scl), d_position=self.n(p["position"].grad),
                    d_cubic=self.n(dc), d_rotation=self.n(p["rotation"].grad), d_opacity=self.n(p["opacity"].grad),
                    d_scaling=self.n(p["scaling"].grad))

    def ppf(self, c, t):
        from splatter_a_video_amd import dynamics as dy
        p = [self.t(c[k], True) for k in ("position", "pos_poly", "pos_fourier")]
        pos = dy.position_poly_fourier(c["clock"], t, p[0], p[1], p[2])
        (pos * self.t(c["g_pos"])).sum().backward()
        return dict(pos=self.n(pos), d_position=self.n(p[0].grad), d_poly=self.n(p[1].grad), d_fourier=self.n(p[2].grad))

    def frame_preprocess(self, c, t, layout):
        from splatter_a_video_amd import dynamics as dy
        N, I = c["N"], c["I"]
        p = {k: self.t(c[k], True) for k in ("position", "rotation", "opacity", "scaling")}
        cub = self.t(c["cubic"])
        cub = (dy.to_segment_major(cub, I) if layout == tw.SEGMENT_MAJOR else cub).requires_grad_(True)
        uv, d, conic, radius, tiles, opa = dy.frame_preprocess(
            c["clock"], t, self.t(c["extr"]), c["W"], c["H"], position=p["position"], pos_cubic_node=cub, rotation=p["rotation"],
            rot_poly_feat=self.t(c["rot_poly"]), rot_fourier_feat=self.t(c["rot_fourier"]), opacity=p["opacity"],
            scaling=p["scaling"], nearest=c["nearest"], extent=c["extent"], cubic_layout=layout)
        ((uv.nan_to_num() * self.t(c["g_uv"])).sum() + (d * self.t(c["g_d"])).sum() + (conic * self.t(c["g_conic"])).sum()
         + (opa * self.t(c["g_opa"])).sum()).backward()
        dc = cub.grad
        dc = dy.to_gaussian_major(dc) if layout == tw.SEGMENT_MAJOR else dc.reshape(N, -1)
        return dict(uv=self.n(uv), depth=self.n(d), conic=self.n(conic), radius=self.n(radius), tiles=self.n(tiles), opa=self.n(opa),
                    d_position=self.n(p["position"].grad), d_cubic=self.n(dc), d_rotation=self.n(p["rotation"].grad),
                    d_opacity=self.n(p["opacity"].grad), d_scaling=self.n(p["scaling"].grad))
